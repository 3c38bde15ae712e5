"""Case tables of the kernel-selection arms (tests/test_gpu_dispatch_arms.py runs them on the GPU,
tests/test_host.py proves on the CPU that they cover every arm).

The C entry points choose among many kernel instantiations by shape and dtype; the library reports each
choice through a host-only query (lss_splat_bwd_arm, lss_lift_prep_arm, lss_dwconv_arm, lss_bn_arm; the
launchers switch on the same functions). Every case here carries its arguments and the arm it is meant to hit.
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
# Batch norm (its own bars, derived at bn_map_bar / bn_fwd_bars below), the largest case of each family, numpy's
# pairwise order | one element after the other; per-channel outputs with BN_K = 64, BN_K_SQ = 512:
#   one group, 16,384 elements a channel:   save_mean 0.007 | 0.144, rstd 0.001 | 0.093, dbeta / dgamma 0.000 | 0.009
#   two-pass and cluster, 32,800 / 32,768:  save_mean 0.012 | 0.143, rstd 0.002 | 0.218, dbeta / dgamma 0.000 | 0.010
#   NHWC, 2,048 rows:                       save_mean 0.010 | 0.010, rstd 0.001 | 0.032, dbeta / dgamma 0.001 | 0.007
#   fp32 maps against rtol = atol = 1e-4:   y 0.008 | 0.873 (through the sequentially summed statistics), dx 0.002
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


# ----------------------------------------------------------------------------- batch norm
# lss_bn_arm's passes, families and names (include/lss_convs.h)
BN_FWD, BN_BWD, BN_EVAL = 0, 1, 2
BN_FAMILIES = ("nhwc", "cluster", "fused_reg", "fused", "two_pass", "eval_nchw", "eval_nhwc")
ACT = {"none": 0, "relu": 1, "swish": 2}
BN_EPS, BN_MOM = 1e-3, 0.1
BN_SEED = 100000  # (committed with the draws: test_host.py's caps and left-out-element proofs hold for this one)


def bn_arm_name(family: int, v: int, it: int, relu: int) -> str:
    """lss_bn_arm_t as the table writes it."""
    name = BN_FAMILIES[family]
    if name == "cluster":
        return "cluster<%d,%d%s>" % (v, it, ",relu" if relu else "")
    if name == "fused_reg":
        return "fused_reg<%d,%d>" % (v, it)
    return name if name.endswith("nhwc") else "%s<%d>" % (name, v)


def bn_arms(pas: int, dtype) -> set:
    """Every training arm include/lss_convs.h enumerates for a pass and dtype."""
    arms = {"nhwc"} | {"%s<%d>" % (f, v) for f in ("fused", "two_pass") for v in (8, 4, 1)}
    if dtype == BF16:
        arms |= {"fused_reg<8,4>", "fused_reg<8,5>", "fused_reg<8,8>", "fused_reg<4,4>", "fused_reg<4,8>",
                 "cluster<8,6>", "cluster<8,8>"}
        if pas == BN_BWD:
            arms |= {"cluster<8,6,relu>", "cluster<8,8,relu>"}
    return arms


# (N, C, H, W), layout (0 NCHW, 1 NHWC), ngroups, whether a sync workspace is passed; the arm the forward takes
# with fp32 / bf16 maps, the backward's where it differs (bwd: a (f32, bf16) pair or None); py: the shape also runs
# through norm.bn_act, where lss_bn_groups must pick this ngroups
BnCase = namedtuple("BnCase", "N C H W layout G sync f32 bf16 bwd py note", defaults=(None, False, ""))
_T8, _T4, _T1 = "two_pass<8>", "two_pass<4>", "two_pass<1>"
BN_CASES = [
    # ---- NCHW, one group, C = 3: both sides of every bound on cnt = N * HW / V (bf16: the register kernels)
    BnCase(2, 3, 32, 128, 0, 1, True, "fused<8>", "fused_reg<8,4>", py=True, note="cnt 1024: every register full"),
    BnCase(93, 3, 8, 11, 0, 1, True, "fused<8>", "fused_reg<8,4>", note="cnt 1023, 11 vectors an image"),
    BnCase(25, 3, 8, 41, 0, 1, True, "fused<8>", "fused_reg<8,5>", py=True, note="cnt 1025, 41 vectors an image"),
    BnCase(8, 3, 32, 40, 0, 1, True, "fused<8>", "fused_reg<8,5>", note="cnt 1280: full"),
    BnCase(21, 3, 8, 61, 0, 1, True, "fused<8>", "fused_reg<8,8>", py=True, note="cnt 1281, 61 vectors an image"),
    BnCase(23, 3, 8, 89, 0, 1, True, "fused<8>", "fused_reg<8,8>", py=True, note="cnt 2047: lss_bn_groups' last"),
    BnCase(2, 3, 64, 128, 0, 1, True, "fused<8>", "fused_reg<8,8>", note="cnt 2048 at ngroups 1: full"),
    BnCase(3, 3, 8, 683, 0, 1, True, "fused<8>", "fused<8>", note="cnt 2049 at ngroups 1: generic bf16"),
    BnCase(1024, 3, 2, 2, 0, 1, True, "fused<4>", "fused_reg<4,4>", note="V 4, cnt 1024"),
    BnCase(93, 3, 4, 11, 0, 1, True, "fused<4>", "fused_reg<4,4>", py=True, note="V 4, cnt 1023, 11 vectors an image"),
    BnCase(25, 3, 4, 41, 0, 1, True, "fused<4>", "fused_reg<4,8>", py=True, note="V 4, cnt 1025, 41 vectors an image"),
    BnCase(2048, 3, 2, 2, 0, 1, True, "fused<4>", "fused_reg<4,8>", note="V 4, cnt 2048: full"),
    BnCase(3, 3, 4, 683, 0, 1, True, "fused<4>", "fused<4>", py=True, note="V 4, cnt 2049: generic bf16"),
    BnCase(2, 3, 5, 7, 0, 1, True, "fused<1>", "fused<1>", py=True, note="V 1"),
    # ---- NCHW two-pass: several groups, no workspace; groups of unequal image counts, one image a group
    BnCase(5, 3, 2, 4, 0, 2, False, _T8, _T8, note="groups of 2 and 3 images"),
    BnCase(5, 3, 2, 4, 0, 3, False, _T8, _T8, note="groups of 1, 2, 2"),
    BnCase(5, 3, 2, 4, 0, 5, False, _T8, _T8, note="G = N"),
    BnCase(5, 3, 2, 6, 0, 2, False, _T4, _T4, note="groups of 2 and 3 images"),
    BnCase(5, 3, 2, 6, 0, 3, False, _T4, _T4, note="groups of 1, 2, 2"),
    BnCase(5, 3, 2, 6, 0, 5, False, _T4, _T4, note="G = N"),
    BnCase(5, 3, 3, 5, 0, 2, False, _T1, _T1, note="groups of 2 and 3 images"),
    BnCase(5, 3, 3, 5, 0, 3, False, _T1, _T1, note="groups of 1, 2, 2"),
    BnCase(5, 3, 3, 5, 0, 5, False, _T1, _T1, note="G = N"),
    BnCase(65, 3, 1, 3, 0, 65, False, _T1, _T1, note="65 groups: fold_groups' second lap"),
    BnCase(2, 3, 2, 4, 0, 3, False, _T8, _T8, note="ngroups > N: an empty group"),
    BnCase(4, 2, 50, 82, 0, 2, True, _T4, _T4, py=True, note="lss_bn_groups' first G > 1 at V 4"),
    BnCase(5, 2, 65, 63, 0, 2, True, _T1, _T1, py=True, note="lss_bn_groups' first G > 1 at V 1"),
    # ---- NCHW cluster (bf16, V 8, a workspace) and what it refuses
    BnCase(4, 3, 64, 96, 0, 2, True, _T8, "cluster<8,6>", note="6 vectors a thread: full"),
    BnCase(4, 3, 8, 769, 0, 2, True, _T8, "cluster<8,8>", note="1538 vectors: first of <8,8>"),
    BnCase(4, 3, 64, 128, 0, 2, True, _T8, "cluster<8,8>", note="8 vectors a thread: full"),
    BnCase(4, 3, 8, 1025, 0, 2, True, _T8, _T8, note="2050 vectors: past the registers"),
    BnCase(5, 3, 48, 96, 0, 2, True, _T8, "cluster<8,8>", py=True, note="groups of 2 and 3 images, 7 vectors"),
    BnCase(4, 3, 2, 4, 0, 2, True, _T8, "cluster<8,6>", note="N / G = 2"),
    BnCase(3, 3, 2, 4, 0, 2, True, _T8, _T8, note="refused: N / G < 2"),
    BnCase(128, 3, 2, 4, 0, 64, True, _T8, "cluster<8,6>", note="G = 64"),
    BnCase(130, 3, 2, 4, 0, 65, True, _T8, _T8, note="refused: G = 65"),
    BnCase(4, 3, 2, 4, 0, 2, False, _T8, _T8, note="refused: no workspace"),
    BnCase(4, 3, 2, 6, 0, 2, True, _T4, _T4, note="refused: V 4"),
    BnCase(4, 512, 2, 4, 0, 2, True, _T8, "cluster<8,6>", note="C G = 1024"),
    BnCase(4, 513, 8, 8, 0, 2, True, _T8, _T8, bwd=(_T8, "cluster<8,6>"), note="C G = 1026: forward two-pass"),
    BnCase(4, 1152, 2, 4, 0, 2, True, _T8, _T8, bwd=(_T8, "cluster<8,6>"), note="C G = 2304"),
    BnCase(4, 1153, 2, 4, 0, 2, True, _T8, _T8, note="C G = 2306: both two-pass"),
    # ---- NHWC: C / 8 = 1, 2, 8, 64, 256 octets a row; rows M = N H W below one pass of the block, no multiple
    # of the unrolled pass, one exact multiple; ngroups 1, 2, 17, 1025 and more groups than rows
    BnCase(5, 8, 1, 7, 1, 1, False, "nhwc", "nhwc", note="35 rows < 256 a pass"),
    BnCase(3, 8, 7, 49, 1, 2, False, "nhwc", "nhwc", note="1029 rows"),
    BnCase(2, 8, 32, 32, 1, 1, False, "nhwc", "nhwc", note="2048 rows = 2 unrolled passes"),
    BnCase(3, 8, 7, 49, 1, 17, False, "nhwc", "nhwc", note="17 groups"),
    BnCase(3, 8, 7, 49, 1, 1025, False, "nhwc", "nhwc", note="1025 groups: the fold's batched loop and its tail"),
    BnCase(5, 8, 1, 7, 1, 1025, False, "nhwc", "nhwc", note="ngroups > rows: empty groups"),
    BnCase(5, 16, 1, 7, 1, 2, False, "nhwc", "nhwc", py=False, note="35 rows < 128 a pass"),
    BnCase(3, 16, 7, 49, 1, 17, False, "nhwc", "nhwc", note="1029 rows"),
    BnCase(2, 16, 16, 32, 1, 1, False, "nhwc", "nhwc", note="1024 rows = 2 unrolled passes"),
    BnCase(1, 64, 3, 5, 1, 1, False, "nhwc", "nhwc", note="15 rows < 32 a pass"),
    BnCase(3, 64, 7, 49, 1, 2, False, "nhwc", "nhwc", note="1029 rows"),
    BnCase(3, 64, 7, 49, 1, 17, False, "nhwc", "nhwc", note="17 groups"),
    BnCase(2, 64, 8, 16, 1, 1, False, "nhwc", "nhwc", note="256 rows = 2 unrolled passes"),
    BnCase(1, 512, 1, 3, 1, 1, False, "nhwc", "nhwc", note="a wave of octets: 3 rows < 4 a pass"),
    BnCase(5, 512, 1, 7, 1, 2, False, "nhwc", "nhwc", note="35 rows"),
    BnCase(5, 512, 1, 7, 1, 17, False, "nhwc", "nhwc", note="17 groups"),
    BnCase(2, 512, 4, 4, 1, 1, False, "nhwc", "nhwc", note="32 rows = 2 unrolled passes"),
    BnCase(1, 2048, 1, 3, 1, 1, False, "nhwc", "nhwc", note="one row a pass: 3 rows"),
    BnCase(5, 2048, 1, 7, 1, 2, False, "nhwc", "nhwc", note="35 rows"),
    BnCase(1, 2048, 1, 5, 1, 17, False, "nhwc", "nhwc", note="ngroups > rows"),
    BnCase(2, 2048, 2, 2, 1, 1, False, "nhwc", "nhwc", note="8 rows = 2 unrolled passes"),
]
# (case note of the lower neighbour, of the upper neighbour, dtype, pass): the two sides of each bound of the rule
BN_BOUNDARIES = [
    ("cnt 1024: every register full", "cnt 1025, 41 vectors an image", BF16, BN_FWD),
    ("cnt 1280: full", "cnt 1281, 61 vectors an image", BF16, BN_FWD),
    ("cnt 2048 at ngroups 1: full", "cnt 2049 at ngroups 1: generic bf16", BF16, BN_BWD),
    ("V 4, cnt 1024", "V 4, cnt 1025, 41 vectors an image", BF16, BN_FWD),
    ("V 4, cnt 2048: full", "V 4, cnt 2049: generic bf16", BF16, BN_BWD),
    ("6 vectors a thread: full", "1538 vectors: first of <8,8>", BF16, BN_FWD),
    ("8 vectors a thread: full", "2050 vectors: past the registers", BF16, BN_BWD),
    ("N / G = 2", "refused: N / G < 2", BF16, BN_FWD),
    ("G = 64", "refused: G = 65", BF16, BN_FWD),
    ("C G = 1024", "C G = 1026: forward two-pass", BF16, BN_FWD),
    ("C G = 2304", "C G = 2306: both two-pass", BF16, BN_BWD),
    ("N / G = 2", "refused: no workspace", BF16, BN_FWD),
    ("N / G = 2", "refused: V 4", BF16, BN_BWD),
]

# act, residual, y: "y" = given; "null" = the forward without an apply pass / the ReLU backward recomputing y
BnCombo = namedtuple("BnCombo", "act res y")
BN_COMBOS_CLUSTER = [BnCombo(a, r, "y") for a in ("none", "swish", "relu") for r in (False, True)]
BN_COMBOS_NCHW = [BnCombo("swish", False, "y"), BnCombo("relu", True, "y")]
BN_COMBOS_NHWC = [BnCombo("swish", False, "y"), BnCombo("relu", True, "y"), BnCombo("relu", False, "y"),
                  BnCombo("relu", False, "null")]


def bn_combos(case, pas: int):
    """The activation / residual combinations a case runs with. The backward of swish with a residual does not
    exist (the kernels recompute the pre-activation from x alone): lss_bn_bwd2 refuses it."""
    if case.layout == 1:
        return BN_COMBOS_NHWC
    if "cluster" in case.bf16 or (case.bwd and "cluster" in case.bwd[1]):
        return [c for c in BN_COMBOS_CLUSTER if not (pas == BN_BWD and c.act == "swish" and c.res)]
    return BN_COMBOS_NCHW


def bn_case_arm(case, dtype, pas: int, act: str = "none") -> str:
    name = (case.bwd if pas == BN_BWD and case.bwd else (case.f32, case.bf16))[0 if dtype == F32 else 1]
    if pas == BN_BWD and act == "relu" and name.startswith("cluster"):
        name = name[:-1] + ",relu>"
    return name


def bn_id(case) -> str:
    return "%dx%dx%dx%d-%s-G%d%s" % (case.N, case.C, case.H, case.W, ("nchw", "nhwc")[case.layout], case.G,
                                      "-sync" if case.sync else "")


def bn_ranges(case):
    """[(first, last)] element ranges along the reduced axis of the (C, N * HW) view, one per group."""
    HW = case.H * case.W
    M = case.N * HW
    unit = 1 if case.layout == 1 else HW  # NHWC groups cut rows, NCHW groups cut images
    n = M // unit
    cuts = [n * q // case.G * unit for q in range(case.G + 1)]
    return [(a, b - 1) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]


def bn_pinned(case) -> bool:
    """Whether bn_inputs pins the ends of every group's range (at most a 16th of the elements: more of them
    at one value would pull the channel's mean to it)."""
    return 32 * len(bn_ranges(case)) <= case.N * case.H * case.W


def bn_inputs(case, dtype, combo):
    """x, residual, dy as (C, M) float64 arrays of values exact in dtype (M = N H W, image-major), and gamma,
    beta, running mean / var (fp32 values, every channel its own). x = 2 randn + 3. Where bn_pinned, the first
    and the last element of every group's range sit 2 standard deviations of the channel's draw above its mean,
    the channel's very first element (always) 2 below ( at least one of the channel's, test_host.py asserts) with
    dy >= 1 and a residual >= 0, so a kernel that drops a range's last element shows in the sums whatever the
    activation."""
    C, M = case.C, case.N * case.H * case.W
    rng = np.random.default_rng(BN_SEED + case.N * 7919 + C * 131 + M + 17 * case.G + case.layout)
    x = (2.0 * rng.standard_normal((C, M)) + 3.0).astype(np.float32)
    res = rng.standard_normal((C, M)).astype(np.float32)
    dy = rng.standard_normal((C, M)).astype(np.float32)
    gamma = (0.5 + rng.random(C)).astype(np.float32)
    beta = (0.1 * rng.standard_normal(C)).astype(np.float32)
    rm = rng.standard_normal(C).astype(np.float32)
    rv = (0.5 + rng.random(C)).astype(np.float32)
    if bn_pinned(case):
        ends = np.unique(np.array(bn_ranges(case)).reshape(-1))
        x[:, ends] = (x.mean(axis=1) + 2.0 * x.std(axis=1))[:, None]
        res[:, ends] = np.abs(res[:, ends])
        dy[:, ends] = 1.0 + np.abs(dy[:, ends])  # (one sign: the groups' left-out ends cannot cancel)
    # K, the shift of the kernels' sums: an element equal to it adds nothing to them
    # (a multiple of 1/2: x - K then stays on x's own bf16 grid)
    x[:, 0] = np.floor(2.0 * (x[:, 1:].mean(axis=1) - 2.0 * x[:, 1:].std(axis=1))) / 2.0 if M > 2 else 0.0
    r64 = lambda a: rounded(a, dtype).double().numpy()
    return dict(x=r64(x), res=r64(res) if combo.res else None, dy=r64(dy), gamma=gamma.astype(np.float64),
                beta=beta.astype(np.float64), rm=rm.astype(np.float64), rv=rv.astype(np.float64))


def _act_and_slope(z, act: str, ft):
    if act == "relu":
        return np.maximum(z, ft(0)), (z > 0).astype(z.dtype)
    if act == "swish":
        s = ft(1) / (ft(1) + np.exp(-z))
        return z * s, s * (ft(1) + z * (ft(1) - s))
    return z, np.ones_like(z)


def _sum(a, order: str):
    """Row sums of a (C, M) array: numpy's pairwise summation, or one element after the other."""
    a = np.ascontiguousarray(a)  # (rows contiguous: what makes numpy's sum pairwise)
    return a.sum(axis=1) if order == "pairwise" else np.cumsum(a, axis=1)[:, -1]


def bn_reference(ins, combo, dtype, ft=np.float64, order="pairwise", drop=None, fed=None):
    """Training batch norm + activation, forward and backward, restated in numpy (ft = float64: the reference;
    float32 in either summation order: what test_host.py measures the bars' room with).
      forward  mean, biased var, rstd = (var + eps)^-1/2, scale = gamma rstd, shift = beta - mean scale;
               running <- (1 - m) running + m (mean | var n / (n - 1)); y = act(x scale + shift [+ r])
      backward from y ROUNDED to dtype and the statistics rounded to fp32 (what the kernels are handed):
               g = dy act'(.), dbeta = sum g, dgamma = sum g xhat, dx = scale (g - mean g - xhat mean(g xhat)),
               dres = g
    The sums are taken as the kernels document them: of x - K and (x - K)^2 with K the channel's first element.
    drop: element indices left out of every sum (n unchanged): the reference of a kernel that skips them.
    fed: a reference whose y and statistics the backward takes instead of this evaluation's own forward's (what
    the GPU tests hand the backward kernels: the fp64 reference's).
    Returns the outputs and, per sum, the sum of |summands| (the per-channel bars are made of those)."""
    x, dy, res = ins["x"].astype(ft), ins["dy"].astype(ft), ins["res"]
    gamma, beta = ins["gamma"].astype(ft), ins["beta"].astype(ft)
    C, M = x.shape
    n = ft(M)
    keep = np.ones(M, dtype=bool)
    if drop is not None:
        keep[drop] = False
    kk = x[:, :1]
    d = (x - kk)[:, keep]
    s1, s2 = _sum(d, order) / n, _sum(d * d, order) / n
    mean = kk[:, 0] + s1
    var = np.maximum(s2 - s1 * s1, ft(0))
    rstd = ft(1) / np.sqrt(var + ft(BN_EPS))
    scale = gamma * rstd
    shift = beta - mean * scale
    unb = var * n / (n - ft(1)) if M > 1 else var
    run_mean = ft(1 - BN_MOM) * ins["rm"].astype(ft) + ft(BN_MOM) * mean
    run_var = ft(1 - BN_MOM) * ins["rv"].astype(ft) + ft(BN_MOM) * unb
    z = x * scale[:, None] + shift[:, None]
    if res is not None:
        z = z + res.astype(ft)
    y, _ = _act_and_slope(z, combo.act, ft)
    out = dict(mean=mean, var=var, rstd=rstd, scale=scale, shift=shift, run_mean=run_mean, run_var=run_var, y=y, z=z,
               abs_mean=np.abs(x[:, keep]).sum(axis=1) / n,
               abs_var=(d * d).sum(axis=1) / n + s1 * s1 + var)
    # the backward's inputs: the reference's y and statistics as stored
    if fed is not None:
        stats, y_in = fed["stats_in"].astype(ft), fed["y_in"].astype(ft)
    else:
        stats = np.stack([mean, rstd, scale, shift]).astype(np.float32).astype(ft)
        y_in = rounded(y.astype(np.float64), dtype).double().numpy().astype(ft)
    m_, r_, sc_, sh_ = stats
    xhat = (x - m_[:, None]) * r_[:, None]
    if combo.act == "relu":
        slope = (y_in > 0).astype(ft)
    else:
        slope = _act_and_slope(x * sc_[:, None] + sh_[:, None], combo.act, ft)[1]
    g = dy * slope
    gx = g * xhat
    dbeta, dgamma = _sum(g[:, keep], order), _sum(gx[:, keep], order)
    dx = sc_[:, None] * (g - (dbeta / n)[:, None] - xhat * (dgamma / n)[:, None])
    out.update(stats_in=stats, y_in=y_in, dbeta=dbeta, dgamma=dgamma, dx=dx, dres=g,
               abs_dbeta=np.abs(g[:, keep]).sum(axis=1), abs_dgamma=np.abs(gx[:, keep]).sum(axis=1))
    return out


# Bars. Maps: fp32 the project's rtol = atol = 1e-4; bf16 one bf16 ulp of the reference on top (the kernels compute
# in fp32 and round once). Per-channel fp32 outputs: k 2^-23 (sum |summands| + |want|), the summands from the fp64
# reference, carried through rstd / scale / shift / the running update by their derivatives.
# k: the smallest power of two that leaves a plain fp32 numpy evaluation of bn_reference, in the worse of two
# summation orders (numpy's pairwise, one element after the other), at most 1/4 of the bar at the largest case of
# each family (test_host.py::test_arm_references_fp32_margins asserts both that it does and that k / 2 does not).
# One element after the other loses n 2^-24 of a sum of n squares and about sqrt(n) 2^-24 of a sum of signed
# terms, so there are two: BN_K for the plain sums (save_mean, running mean, dbeta, dgamma) and BN_K_SQ for what
# hangs on the sum of squares (rstd, scale, shift, running var). The measured ratios are in the comment block at
# the top of this file. (The backward of that evaluation is handed the fp64 reference's statistics, as the kernels
# are. With BN_K / 2 save_mean takes 0.29 of its bar, with BN_K_SQ / 2 rstd 0.44.)
BN_K = 64
BN_K_SQ = 512
U23 = 2.0 ** -23
BN_RECOMPUTE_EPS = 1e-4  # NHWC ReLU with y = NULL: pre-activations this close to 0 may flip the recomputed mask
BN_RECOMPUTE_CAP = 1e-3  # ... and at most this fraction of a case's elements may be that close


def bn_map_bar(want, dtype):
    want = np.abs(want)
    return F32_TOL["atol"] + F32_TOL["rtol"] * want + (2.0 ** -8 * want if dtype == BF16 else 0.0)


def bn_fwd_bars(ref, ins, k=BN_K, k_sq=BN_K_SQ):
    """Per-channel bars of save_mean, rstd, scale, shift, running mean and running var."""
    e, e2 = k * U23, k_sq * U23
    a = lambda v: np.abs(v)
    mean = e * (ref["abs_mean"] + a(ref["mean"]))
    var = e2 * (ref["abs_var"] + a(ref["var"])) + 2 * a(ref["mean"] - ins["x"][:, 0]) * mean
    rstd = 0.5 * ref["rstd"] / (ref["var"] + BN_EPS) * var + e * ref["rstd"]
    scale = a(ins["gamma"]) * rstd + e * a(ref["scale"])
    shift = a(ref["mean"]) * scale + a(ref["scale"]) * mean + e * (a(ins["beta"]) + a(ref["mean"] * ref["scale"]))
    M = ins["x"].shape[1]
    unb = M / (M - 1.0) if M > 1 else 1.0
    run_mean = BN_MOM * mean + e * ((1 - BN_MOM) * a(ins["rm"]) + BN_MOM * a(ref["mean"]) + a(ref["run_mean"]))
    run_var = BN_MOM * unb * var + e * ((1 - BN_MOM) * a(ins["rv"]) + BN_MOM * unb * ref["var"] + a(ref["run_var"]))
    return dict(mean=mean, rstd=rstd, scale=scale, shift=shift, run_mean=run_mean, run_var=run_var)


def bn_near_zero(ref, combo):
    """(C, M) mask of the elements whose ReLU mask the recomputing backward may legitimately flip."""
    if combo.act == "relu" and combo.y == "null":
        return np.abs(ref["z"]) < BN_RECOMPUTE_EPS
    return np.zeros(ref["z"].shape, dtype=bool)


def bn_bwd_bars(ref, ins, combo, k=BN_K):
    """Per-channel bars of dbeta and dgamma (with the summands of the elements bn_near_zero leaves out)."""
    e = k * U23
    near = bn_near_zero(ref, combo)
    xhat = (ins["x"] - ref["stats_in"][0][:, None]) * ref["stats_in"][1][:, None]
    extra_b = (np.abs(ins["dy"]) * near).sum(axis=1)
    extra_g = (np.abs(ins["dy"] * xhat) * near).sum(axis=1)
    return dict(dbeta=e * (ref["abs_dbeta"] + np.abs(ref["dbeta"])) + extra_b,
                dgamma=e * (ref["abs_dgamma"] + np.abs(ref["dgamma"])) + extra_g)


# ----------------------------------------------------------------------------- squeeze-excite
# lss_se_arm's passes, settings and classes (include/lss_convs.h)
SE_FWD, SE_BWD = 0, 1
SE_OFF, SE_DEFAULT, SE_FORCED = 0, 1, 2  # lss_se_tails
SE_FWD_CHUNKS = ("one_chunk", "chunks", "two_passes")
SE_BWD_CHUNKS = ("one_chunk", "unit_a_wave", "units_a_wave", "two_passes")
SE_BANK_IMAGES = 4096  # LSS_SE_TAIL_MAX_IMAGES
SE_SEED = 180000  # (committed with the draws: test_host.py's left-out-term proofs hold for this one)

# N, C, HW, sq; setting: SE_DEFAULT marks a routing case (it runs under all three settings, the others under 0 and 2)
SeCase = namedtuple("SeCase", "N C HW sq setting note")
_R, _T = SE_DEFAULT, SE_FORCED
SE_CASES = [
    # ---- routing under the default setting: C * sq against 1024 (forward) and 4096 (backward); N against the bank
    SeCase(2, 256, 4, 4, _R, "C sq 1024: forward tail; one plane a wave, full blocks; C 256"),
    SeCase(2, 41, 4, 25, _R, "C sq 1025: forward sequence"),
    SeCase(2, 64, 8, 64, _R, "C sq 4096: backward tail; C 64, sq 64"),
    SeCase(2, 241, 4, 17, _R, "C sq 4097: backward sequence; sq 17"),
    SeCase(4096, 4, 4, 1, _R, "N 4096: the last image of the bank"),
    SeCase(4097, 4, 4, 1, _R, "N 4097: past the bank, the sequence under every setting"),
    # ---- tail grid: planes a wave 1 .. 5, each with full and with ragged blocks
    SeCase(3, 6, 4, 1, _T, "one plane, ragged: a block must not straddle images"),
    SeCase(64, 256, 4, 2, _T, "two planes a wave, full"),
    SeCase(48, 240, 8, 10, _T, "two planes a wave, a last block of one"),
    SeCase(64, 384, 4, 2, _T, "three planes a wave, full"),
    SeCase(64, 376, 4, 2, _T, "three planes a wave, ragged"),
    SeCase(64, 512, 4, 2, _T, "four planes a wave, full"),
    SeCase(64, 500, 4, 2, _T, "four planes a wave, ragged"),
    SeCase(128, 320, 4, 5, _T, "five planes a wave, full: mean 4 + 1, dot 2 + 2 + 1"),
    SeCase(128, 310, 4, 5, _T, "five planes a wave, ragged"),
    SeCase(600, 40, 4, 2, _T, "N 600: one block an image"),
    SeCase(256, 20, 4, 1, _T, "N 256: the last count with two slots an image"),
    SeCase(257, 20, 4, 1, _T, "N 257: one block an image from here on"),
    SeCase(64, 1152, 4, 48, _T, "144 channels a block: mean 4 + 4 + 1, dot 2 + 2 + 2 + 2 + 1"),
    SeCase(40, 600, 12, 25, _T, "64 channels a block, 24 in the last; HW 12"),
    # ---- reduce conv: C around the wave (64), the four-way unrolled loop (193) and the expand chunk (256); sq with
    # rows past the last in the tail's four-row batches
    SeCase(2, 63, 4, 1, _T, "C 63, sq 1"),
    SeCase(2, 64, 4, 3, _T, "C 64, sq 3"),
    SeCase(2, 65, 4, 5, _T, "C 65, sq 5"),
    SeCase(2, 192, 4, 16, _T, "C 192, sq 16"),
    SeCase(2, 193, 4, 17, _T, "C 193, sq 17"),
    SeCase(2, 257, 4, 63, _T, "C 257, sq 63"),
    SeCase(2, 72, 12, 3, _T, "C 72: a second 64-channel chunk of 8 channels"),
    SeCase(2, 320, 8, 5, _T, "C 320: two expand chunks of the sequence, five backward chunks"),
    # ---- expand conv in the tail: the chunk is min(1024, 16384 / (sq + 1)) channels
    SeCase(1, 1025, 4, 15, _T, "sq 15, C 1025: two chunks, the second of one channel"),
    SeCase(1, 963, 4, 16, _T, "sq 16, C 963: one chunk of 963"),
    SeCase(1, 964, 4, 16, _T, "sq 16, C 964: a second chunk of one channel"),
    SeCase(1, 1024, 4, 15, _T, "sq 15, C 1024: one chunk, one pass"),
    SeCase(1, 2048, 4, 64, _T, "the ABI's limits: nine chunks, 128 units"),
    SeCase(5, 1152, 44, 48, _T, "the widest trunk block at its real plane"),
    # ---- planes: a lane's second trip (HW > 256) and a trip that stops mid-wave
    SeCase(2, 5, 252, 2, _T, "HW 252: the last lane idle"),
    SeCase(3, 4, 256, 1, _T, "HW 256: one full trip"),
    SeCase(2, 7, 260, 3, _T, "HW 260: lane 0 makes a second trip"),
    SeCase(2, 3, 516, 2, _T, "HW 516: a third trip"),
    SeCase(48, 8, 4, 2, _T, "the workload's image count"),
    SeCase(1, 4, 4, 1, _T, "one block is the whole image"),
]
# (note below, note above, pass, setting): the two sides of each bound; they fall in different classes
SE_BOUNDARIES = [
    ("C sq 1024: forward tail; one plane a wave, full blocks; C 256", "C sq 1025: forward sequence", SE_FWD, SE_DEFAULT),
    ("C sq 4096: backward tail; C 64, sq 64", "C sq 4097: backward sequence; sq 17", SE_BWD, SE_DEFAULT),
    ("N 4096: the last image of the bank", "N 4097: past the bank, the sequence under every setting", SE_FWD, SE_FORCED),
    ("N 4096: the last image of the bank", "N 4097: past the bank, the sequence under every setting", SE_BWD, SE_DEFAULT),
    ("N 256: the last count with two slots an image", "N 257: one block an image from here on", SE_FWD, SE_FORCED),
    ("sq 16, C 963: one chunk of 963", "sq 16, C 964: a second chunk of one channel", SE_FWD, SE_FORCED),
    ("sq 15, C 1024: one chunk, one pass", "sq 15, C 1025: two chunks, the second of one channel", SE_FWD, SE_FORCED),
    ("sq 15, C 1024: one chunk, one pass", "sq 15, C 1025: two chunks, the second of one channel", SE_BWD, SE_FORCED),
    ("C sq 1024: forward tail; one plane a wave, full blocks; C 256", "C 257, sq 63", SE_FWD, SE_OFF),
    ("C sq 1024: forward tail; one plane a wave, full blocks; C 256", "C 257, sq 63", SE_BWD, SE_FORCED),
    ("C 64, sq 3", "C 65, sq 5", SE_BWD, SE_OFF),
    ("C 64, sq 3", "C 65, sq 5", SE_BWD, SE_FORCED),
    ("two planes a wave, full", "three planes a wave, full", SE_FWD, SE_FORCED),
    ("three planes a wave, full", "four planes a wave, full", SE_BWD, SE_FORCED),
    ("four planes a wave, full", "five planes a wave, full: mean 4 + 1, dot 2 + 2 + 1", SE_FWD, SE_FORCED),
    ("three planes a wave, full", "three planes a wave, ragged", SE_FWD, SE_FORCED),
]
# lss_se_wgrad, (N, C, sq): N on either side of the unroll of 16 images; 2 C sq + sq + C no multiple of 256, and with
# C sq = 15 one wave holds all four branches (dw2, dw1, db1, db2)
SE_WGRAD_CASES = [(1, 5, 3), (15, 5, 3), (16, 5, 3), (17, 100, 7), (33, 5, 3), (33, 100, 7)]
SE_AUTOGRAD = ("C 72: a second 64-channel chunk of 8 channels", "two planes a wave, a last block of one",
               "HW 260: lane 0 makes a second trip")


def se_id(c) -> str:
    return "%dx%dx%d-sq%d" % (c.N, c.C, c.HW, c.sq)


def se_case(note: str):
    return next(c for c in SE_CASES if c.note == note)


def se_settings(c):
    return (SE_OFF, SE_DEFAULT, SE_FORCED) if c.setting == SE_DEFAULT else (SE_OFF, SE_FORCED)


def se_class(pas: int, a) -> tuple:
    """lss_se_arm_t as a class: (path, planes a wave, ragged, one block an image, chunk class)."""
    chunk = (SE_BWD_CHUNKS if pas == SE_BWD else SE_FWD_CHUNKS)[a.chunk_class]
    return ("tails" if a.tails else "sequence", a.planes_class, bool(a.ragged), a.tails == 1 and a.bpi == 1, chunk)


def se_classes(pas: int, tails: bool) -> dict:
    """What include/lss_convs.h enumerates for a pass and path, axis by axis."""
    chunks = set(SE_BWD_CHUNKS) if pas == SE_BWD else set(SE_FWD_CHUNKS[:3 if tails else 2])
    if tails:
        return dict(planes={(p, r) for p in (1, 2, 3, 4, 5) for r in (False, True)}, one_block={False, True}, chunks=chunks)
    return dict(planes={(1, False), (1, True)}, one_block={False}, chunks=chunks)


def rbf(v):
    """v rounded to the nearest bf16 value, ties to even, as float64 (from float64 directly: no double rounding)."""
    v = np.asarray(v, dtype=np.float64)
    e = np.frexp(v)[1] - 1  # |v| in [2^e, 2^(e + 1))
    return np.where(v == 0, 0.0, np.ldexp(np.rint(np.ldexp(v, 7 - e)), e - 7))


def bf16_half(got, exact):
    """Half the distance from the bf16 value got to its bf16 neighbour on exact's side."""
    got, exact = np.asarray(got, dtype=np.float64), np.asarray(exact, dtype=np.float64)
    f, e = np.frexp(got)
    half = np.ldexp(1.0, e - 1 - 8)
    inward = (np.abs(exact) < np.abs(got)) | (np.sign(exact) != np.sign(got))
    return np.where(got == 0, 0.0, np.where(inward & (np.abs(f) == 0.5), half / 2, half))


def se_inputs(N: int, C: int, HW: int, sq: int):
    """x, dy (N, C, HW): bf16 values with |v| in [0.5, 2] and a random sign (no term of a plane's sum is negligible);
    w1 (sq, C), b1, w2 (C, sq), b2: fp32 masters scaled as test_gpu_se_tails._inputs scales them. All float64 arrays."""
    rng = np.random.default_rng(SE_SEED + 7919 * N + 131 * C + 17 * HW + sq)

    def away(shape):
        v = (0.5 + 1.5 * rng.random(shape)) * np.where(rng.random(shape) < 0.5, -1.0, 1.0)
        return rounded(v, BF16).double().numpy()
    f32 = lambda a: a.astype(np.float32).astype(np.float64)  # noqa: E731
    return dict(x=away((N, C, HW)), dy=away((N, C, HW)),
                w1=f32(rng.standard_normal((sq, C)) / C ** 0.5), b1=f32(rng.standard_normal(sq)),
                w2=f32(rng.standard_normal((C, sq)) / sq ** 0.5), b2=f32(rng.standard_normal(C)))


# Bars. Every stage is recomputed in fp64 from the buffers that feed it, so a bar has to cover one stage's fp32
# arithmetic only. With u = 2^-24 (half an fp32 ulp, the relative error of one rounding) a stage whose every term
# passes through at most d roundings errs by at most d u sum |terms| (first order; d u < 2^-17 throughout). d is read
# from the summation order written in lss_se.hip, and the bar is SE_ROOM d u sum |terms|: the 4x room the batch-norm
# bars are held to, so that a re-associated kernel of the same depth, and test_host.py's fp32 evaluation, still pass.
# Products of two bf16 values are exact in fp32, and an fma rounds once.
#   m     se_plane_mean: per lane and trip (v0 + v1) + (v2 + v3) then s +=: 3 a trip, ceil(HW / 256) trips; the
#         six-step wave tree; the division by HW
#   r     se_fc1_dots: a lane has at most ceil(C / 64) channels, its four partial sums take a quarter of them (rounded
#         down) in the unrolled loop, partial 0 up to 3 more in the remainder loop; (a0 + a1) + (a2 + a3): 2; the wave tree: 6; + b1: 1
#   sigmoid(z) = 1 / (1 + __expf(-z)), __expf(x) = exp2(x log2(e)): the product's rounding and the constant's move the
#         result by |x| u each, the hardware exp2 is good to 1 ulp = 2 u; so exp errs by (2 |z| + 2) u, which 1 + . damps
#         and rounds (1), and the correctly rounded division rounds (1): relative error (2 |z| + 4) u
#   h     r sigmoid(r): the sigmoid's and one product
#   e     se_fc2: sq fmas in sequence (the first onto zero), + b2: sq of them
#   t     se_plane_dot: 4 fmas a trip in one chain, ceil(HW / 256) trips; the wave tree: 6
#   de    t s (1 - s): 1 - s, two products: 3
#   dh_part  se_dh16: a product each (1), 16 added in sequence (15); sum4 of the four waves: 2
#   dr    dh: the above and the chunks' partials added in sequence, ceil(C / 64) more; then dh s (1 + r (1 - s)) with
#         s = sigmoid(r): written out at se_bwd_stages
#   dm    se_dm_range: at most 16 fmas in sequence; sum4: 2
#   dx    fma(g, sig, dm / HW): the division's rounding of dm / HW and the fma's of the sum
#   dw1, db1, dw2, db2   k_se_wgrad: N fmas (or adds) in image order
SE_ROOM = 4
U24 = 2.0 ** -24
SE_D_DE, SE_D_DHP, SE_D_DM = 3, 18, 18


def se_d_m(HW): return 3 * -(-HW // 256) + 6 + 1
def se_d_r(C): return -(-C // 64) // 4 + 3 + 2 + 6 + 1
def se_d_sigmoid(z): return 2 * np.abs(z) + 4
def se_d_e(sq): return sq
def se_d_t(HW): return 4 * -(-HW // 256) + 6
def se_d_dh(C): return SE_D_DHP + -(-C // 64)


def _sigmoid(z):
    return 1 / (1 + np.exp(-z))


def _dot(a, b, order: str):
    """sum_k a[..., k] b[..., k] over the last axis: numpy's pairwise sum of the products, or one after the other."""
    p = np.ascontiguousarray(a * b)
    return p.sum(axis=-1) if order == "pairwise" else np.cumsum(p, axis=-1)[..., -1]


def se_weights(ins):
    """The weights and biases as the kernels use them: rounded to bf16."""
    return rbf(ins["w1"]), rbf(ins["b1"]), rbf(ins["w2"]), rbf(ins["b2"])


def se_reference(ins, ft=np.float64, order="pairwise", fed=None):
    """include/lss_convs.h's squeeze-excite contract restated in numpy, every buffer of the C ABI, with bf16 rounding
    (nearest even) where the header says autocast rounds; pre_*: the value before that rounding. ft = float64: the
    reference. ft = float32 in either order: the evaluation test_host.py measures the bars' room with (it chains its
    own rounded buffers, as the kernels do). fed: the reference whose r, sig the backward and whose de, h, dr, m the
    weight gradients take (what the GPU tests hand lss_se_bwd and lss_se_wgrad); default: this evaluation's own."""
    c = lambda a: np.asarray(a).astype(ft)  # noqa: E731
    x, dy = c(ins["x"]), c(ins["dy"])
    w1, b1, w2, b2 = (c(w) for w in se_weights(ins))
    N, C, HW = x.shape
    o = {}
    o["pre_m"] = _dot(x, np.ones_like(x), order) / ft(HW)
    o["m"] = c(rbf(o["pre_m"]))
    o["pre_r"] = _dot(o["m"][:, None, :], w1[None], order) + b1
    o["r"] = c(rbf(o["pre_r"]))
    o["pre_h"] = o["r"] * _sigmoid(o["r"])
    o["h"] = c(rbf(o["pre_h"]))
    o["pre_e"] = _dot(o["h"][:, None, :], w2[None], order) + b2
    o["e"] = c(rbf(o["pre_e"]))
    o["pre_sig"] = _sigmoid(o["e"])
    o["sig"] = c(rbf(o["pre_sig"]))
    o["y"] = rbf(o["sig"][..., None].astype(np.float64) * ins["x"])
    src = o if fed is None else fed
    r, sig = c(src["r"]), c(src["sig"])
    o["t"] = _dot(dy, x, order)
    o["de"] = o["t"] * sig * (1 - sig)
    nchunk = -(-C // 64)
    pad = np.zeros((N, nchunk * 64 - C), dtype=ft)
    dec = np.concatenate([o["de"], pad], axis=1).reshape(N, nchunk, 64)
    w2c = np.concatenate([w2, np.zeros((nchunk * 64 - C, w2.shape[1]), dtype=ft)]).reshape(nchunk, 64, -1)
    o["dh_part"] = _dot(dec[:, :, None, :], w2c.transpose(0, 2, 1)[None], order)  # (N, nchunk, sq)
    dh = _dot(o["dh_part"].transpose(0, 2, 1), np.ones((1, 1, nchunk), dtype=ft), order)
    s = _sigmoid(r)
    o["dr"] = dh * s * (1 + r * (1 - s))
    o["dm"] = _dot(o["dr"][:, None, :], w1.T[None], order)
    o["pre_dx"] = dy * sig[..., None] + (o["dm"] / ft(HW))[..., None]
    o["dx"] = rbf(o["pre_dx"])
    src = o if fed is None else fed
    de, h, dr, m = (c(np.asarray(src[k]).astype(np.float32)) for k in ("de", "h", "dr", "m"))
    o.update(se_wgrad_reference(de, h, dr, m, ft, order))
    return o


def se_wgrad_reference(de, h, dr, m, ft=np.float64, order="pairwise"):
    c = lambda a: np.asarray(a).astype(ft)  # noqa: E731
    de, h, dr, m = c(de), c(h), c(dr), c(m)
    one = np.ones((1, de.shape[0]), dtype=ft)
    return dict(dw1=_dot(dr.T[:, None, :], m.T[None], order), db1=_dot(dr.T, one, order),
                dw2=_dot(de.T[:, None, :], h.T[None], order), db2=_dot(de.T, one, order))


def se_fwd_stages(ins, buf):
    """name -> (exact, slack) of the forward's stages, each from the buffer before it in buf (m, r, h as the kernel
    or an evaluation stored them): exact in fp64, slack the fp32 part of the bar. e: the hidden bf16(W2 h + b2)."""
    x = ins["x"]
    w1, b1, w2, b2 = se_weights(ins)
    N, C, HW = x.shape
    sq = w1.shape[0]
    k = SE_ROOM * U24
    m, r, h = (np.asarray(buf[n], dtype=np.float64) for n in ("m", "r", "h"))
    out = {"m": (x.mean(axis=-1), k * se_d_m(HW) * np.abs(x).mean(axis=-1))}
    out["r"] = (m @ w1.T + b1, k * se_d_r(C) * (np.abs(m) @ np.abs(w1).T + np.abs(b1)))
    hx = r * _sigmoid(r)
    out["h"] = (hx, k * (se_d_sigmoid(r) + 1) * np.abs(hx))
    out["e"] = (h @ w2.T + b2, k * se_d_e(sq) * (np.abs(h) @ np.abs(w2).T + np.abs(b2)))
    return out


def se_sig_stage(e):
    """(exact, slack) of sig given the bf16 value e."""
    s = _sigmoid(np.asarray(e, dtype=np.float64))
    return s, SE_ROOM * U24 * se_d_sigmoid(e) * s


def se_ratio(got, exact, slack, bf16: bool, beyond: bool = False):
    """|got - exact| over the bar, per element: the bar is slack, plus for a value stored rounded to bf16 half the
    distance to got's bf16 neighbour on exact's side (either neighbour of a near-tie is admitted, nothing else).
    beyond: what the error exceeds that half step by, over slack alone (the fp32 arithmetic's share of the bar: a
    correctly rounded value sits at up to 1.0 of the whole bar, and at 0 of this)."""
    got = np.asarray(got, dtype=np.float64)
    half = bf16_half(got, exact) if bf16 else 0.0
    err = np.abs(got - exact)
    if beyond:
        return np.maximum(err - half, 0.0) / np.maximum(slack, 1e-300)
    return np.where(err == 0, 0.0, err / np.maximum(slack + half, 1e-300))


def se_sig_ratio(got, e_exact, e_slack, beyond: bool = False):
    """sig is admissible if it is for some bf16 e within its bar of the exact e: the candidates are the roundings of
    the two ends of [e_exact - slack, e_exact + slack] (the slack is far below a bf16 step)."""
    ratios = [se_ratio(got, *se_sig_stage(rbf(e_exact + d)), True, beyond) for d in (-e_slack, e_slack)]
    return np.minimum(*ratios)


def se_bwd_stages(ins, fed, buf):
    """The backward's stages, chained like the forward's: t from dy and x; de from buf's t; dh_part and dr from its
    de; dm from its dr; dx from its dm. fed: the reference whose r and sig lss_se_bwd was handed."""
    x, dy = ins["x"], ins["dy"]
    w1, _, w2, _ = se_weights(ins)
    N, C, HW = x.shape
    sq = w1.shape[0]
    k = SE_ROOM * U24
    r, sig = fed["r"].astype(np.float64), fed["sig"].astype(np.float64)
    t, de, dr, dm = (np.asarray(buf[n], dtype=np.float64) for n in ("t", "de", "dr", "dm"))
    out = {"t": ((dy * x).sum(axis=-1), k * se_d_t(HW) * np.abs(dy * x).sum(axis=-1))}
    dex = t * sig * (1 - sig)
    out["de"] = (dex, k * SE_D_DE * np.abs(dex))
    nchunk = -(-C // 64)
    dec = np.concatenate([de, np.zeros((N, nchunk * 64 - C))], axis=1).reshape(N, nchunk, 64)
    w2c = np.concatenate([w2, np.zeros((nchunk * 64 - C, sq))]).reshape(nchunk, 64, sq)
    out["dh_part"] = (np.einsum("nqc,qcj->nqj", dec, w2c), k * SE_D_DHP * np.einsum("nqc,qcj->nqj", np.abs(dec), np.abs(w2c)))
    # dr = dh s F, F = 1 + r (1 - s), s = sigmoid(r) computed with relative error es = se_d_sigmoid(r) u:
    # 1 - s errs by s es + u (1 - s) <= s es + u, the fma r (1 - s) + 1 adds u |F|, the two products 2 u:
    # |d dr| <= |dh| (s |F| (es + 3 u) + s |r| (s es + u)), and dh's own error passes through |s F|
    dh, dh_abs = de @ w2, np.abs(de) @ np.abs(w2)
    s = _sigmoid(r)
    F = 1 + r * (1 - s)
    es = se_d_sigmoid(r)
    out["dr"] = (dh * s * F, k * (se_d_dh(C) * dh_abs * np.abs(s * F)
                                   + np.abs(dh) * (s * np.abs(F) * (es + 3) + s * np.abs(r) * (s * es + 1))))
    out["dm"] = (dr @ w1, k * SE_D_DM * (np.abs(dr) @ np.abs(w1)))
    b = dm / HW
    dxx = dy * sig[..., None] + b[..., None]
    out["dx"] = (dxx, k * (np.abs(b)[..., None] + np.abs(dxx)))
    return out


def se_wgrad_stages(de, h, dr, m):
    """The four gradients from the fp32 de, h, dr, m lss_se_wgrad was handed."""
    de, h, dr, m = (np.asarray(a, dtype=np.float64) for a in (de, h, dr, m))
    k = SE_ROOM * U24 * de.shape[0]
    return {"dw1": (dr.T @ m, k * (np.abs(dr).T @ np.abs(m))), "db1": (dr.sum(axis=0), k * np.abs(dr).sum(axis=0)),
            "dw2": (de.T @ h, k * (np.abs(de).T @ np.abs(h))), "db2": (de.sum(axis=0), k * np.abs(de).sum(axis=0))}


SE_FWD_BF16 = ("m", "r", "h")  # fp32 buffers that hold a bf16 value (and sig, checked through e)


def se_rooms(ins, buf, fed, dh_part: bool = True):
    """Largest |error| / bar of every buffer of one run (buf: name -> array; y and dx as fp64 of their bf16): under 1
    everywhere is the test. y must equal bf16(x sig) of buf's own sig exactly: inf if any element differs."""
    rooms = {}
    f = se_fwd_stages(ins, buf)
    for n in SE_FWD_BF16:
        rooms[n] = float(se_ratio(buf[n], *f[n], True).max())
    rooms["sig"] = float(se_sig_ratio(buf["sig"], *f["e"]).max())
    y = rbf(np.asarray(buf["sig"], dtype=np.float64)[..., None] * ins["x"])
    rooms["y"] = 0.0 if np.array_equal(y, np.asarray(buf["y"], dtype=np.float64)) else np.inf
    b = se_bwd_stages(ins, fed, buf)
    for n in ("t", "de", "dr", "dm") + (("dh_part",) if dh_part else ()):
        rooms[n] = float(se_ratio(buf[n], *b[n], False).max())
    rooms["dx"] = float(se_ratio(buf["dx"], *b["dx"], True).max())
    # the bf16-valued buffers again, the half step taken off: the fp32 arithmetic's share (reported, implied by the above)
    for n in SE_FWD_BF16:
        rooms[n + ">half"] = float(se_ratio(buf[n], *f[n], True, beyond=True).max())
    rooms["sig>half"] = float(se_sig_ratio(buf["sig"], *f["e"], beyond=True).max())
    rooms["dx>half"] = float(se_ratio(buf["dx"], *b["dx"], True, beyond=True).max())
    return rooms


def se_wgrad_rooms(fed4, got):
    st = se_wgrad_stages(*fed4)
    return {n: float(se_ratio(got[n], *st[n], False).max()) for n in st}


def se_wgrad_inputs(N: int, C: int, sq: int):
    """de (N, C), h (N, sq), dr (N, sq), m (N, C) for lss_se_wgrad's own cases: fp32 values, h and m bf16 ones."""
    rng = np.random.default_rng(SE_SEED + 31 * N + 7 * C + sq)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)  # noqa: E731
    return (f32(rng.standard_normal((N, C))), rbf(rng.standard_normal((N, sq))), f32(rng.standard_normal((N, sq))),
            rbf(rng.standard_normal((N, C))))
