"""What the valid-cell mask tests share: lss_simbev_valid_mask restated in numpy, independently of the package --
float32 arrays, the kernel's operation order (numpy rounds every product, sum and quotient once and fuses nothing),
the same tests on the floats --, the float64 construction of the camera blocks, the rigs (the committed fixture's
calibration under a few image augmentations), the grids and the index matrices of the cases."""
import glob
import json
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SMALL = os.path.join(HERE, "golden", "simbev_small")
SRC_HW = (56, 120)          # the fixture's images
FINAL_DIM = (64, 192)
DBOUND = (4.0, 45.0, 1.0)
# (X, Y, cell in metres): the default grid, and the three small ones the GPU tests run -- ragged blocks (256 and 240
# cells: one block, partly empty), rows shorter than a wave
GRIDS = {"200x200": (200, 200, 0.5), "16x16": (16, 16, 6.25), "20x12": (20, 12, 5.0), "5x7": (5, 7, 16.0)}
GPU_GRIDS = ("16x16", "20x12", "5x7")
HEIGHTS = {"one": (0.0,), "three": (0.0, 1.5, -1.0)}
EYE = np.array([[1, 0, 0], [0, 1, 0]], dtype=np.float32)


def grid_conf(X, Y, cell):
    return {"xbound": [-X * cell / 2, X * cell / 2, cell], "ybound": [-Y * cell / 2, Y * cell / 2, cell],
            "zbound": [-10.0, 10.0, 20.0], "dbound": list(DBOUND)}


def grid_args(X, Y, cell):
    """(x0, dx, y0, dy) as the fp32 values the entry is given: the first cell's centre and the cell size."""
    f = np.float32
    return f(-X * cell / 2 + cell / 2), f(cell), f(-Y * cell / 2 + cell / 2), f(cell)


# ----------------------------------------------------------------------------- rigs
def _post(resize, crop, flip, rotate_deg):
    """img_transform's post-homography (src/tools.py:130-142) in float64: (P (2, 2), q (2,))."""
    P = np.eye(2) * resize
    q = -np.array(crop[:2], dtype=np.float64)
    if flip:
        A = np.array([[-1.0, 0.0], [0.0, 1.0]])
        P, q = A @ P, A @ q + np.array([crop[2] - crop[0], 0.0])
    h = math.radians(rotate_deg)
    A = np.array([[math.cos(h), math.sin(h)], [-math.sin(h), math.cos(h)]])
    b = np.array([crop[2] - crop[0], crop[3] - crop[1]]) / 2
    b = A @ (-b) + b
    return A @ P, A @ q + b


# per sample: (resize, bottom fraction, left offset, flip, rotation in degrees); the first is validation's window at
# resize 1.7
AUGS = [(1.7, 0.11, 6, False, 0.0), (1.62, 0.05, 1, True, 4.0), (1.78, 0.2, 17, False, -5.0)]


def golden_rig(n, N=6):
    """The calibration of the fixture's first n samples (float32, as the loader reads it) with AUGS' image
    augmentations: dict of rots (n, N, 3, 3), trans (n, N, 3), intrins, post_rots (n, N, 3, 3), post_trans (n, N, 3)."""
    metas = []
    for f in sorted(glob.glob(os.path.join(SMALL, "SimBEV_cvt_label", "scene_*", "yaw0pitch0", "meta.json"))):
        metas.extend(json.load(open(f)))
    rig = {k: [] for k in ("rots", "trans", "intrins", "post_rots", "post_trans")}
    H, W = SRC_HW
    fH, fW = FINAL_DIM
    for b in range(n):
        s = metas[b]
        resize, bottom, left, flip, rot = AUGS[b % len(AUGS)]
        top = int((1 - bottom) * int(H * resize)) - fH
        P, q = _post(resize, (left, top, left + fW, top + fH), flip, rot)
        pr, pt = np.eye(3), np.zeros(3)
        pr[:2, :2], pt[:2] = P, q
        ext = np.array(s["extrinsics"], dtype=np.float64)[:N]
        rig["rots"].append(ext[:, :3, :3])
        rig["trans"].append(ext[:, :3, 3])
        rig["intrins"].append(np.array(s["intrinsics"], dtype=np.float64)[:N])
        rig["post_rots"].append(np.stack([pr] * N))
        rig["post_trans"].append(np.stack([pt] * N))
    return {k: np.stack(v).astype(np.float32) for k, v in rig.items()}


def compose(rig, A):
    """The rig under the BEV-space augmentation p' = A p (A (n, 3, 3) float32): rots' = A rots, trans' = A trans, fp32."""
    out = dict(rig)
    out["rots"] = np.einsum("bij,bnjk->bnik", A, rig["rots"]).astype(np.float32)
    out["trans"] = np.einsum("bij,bnj->bni", A, rig["trans"]).astype(np.float32)
    return out


def cameras64(rig):
    """(cams (n, N, 16), q (n, N, 2)) in float64 from the float32 rig: M = K R^-1, o = -M t, P, and post_trans[:2]."""
    R, t = rig["rots"].astype(np.float64), rig["trans"].astype(np.float64)
    K, pr = rig["intrins"].astype(np.float64), rig["post_rots"].astype(np.float64)
    M = K @ np.linalg.inv(R)
    o = -np.einsum("bnij,bnj->bni", M, t)
    lead = M.shape[:2]
    return (np.concatenate([M.reshape(*lead, 9), o, pr[..., :2, :2].reshape(*lead, 4)], axis=-1),
            rig["post_trans"].astype(np.float64)[..., :2])


# ----------------------------------------------------------------------------- index matrices
def index_matrix(theta_deg, scale, flip_x, flip_y, X, Y, cell):
    """label_index_matrix restated: M = D^-1 A2^-1 D, b = D^-1 (A2^-1 lo - lo), float64, rounded once; and A (3, 3)."""
    t = math.radians(theta_deg)
    c, s = math.cos(t), math.sin(t)
    A = scale * (np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]) @ np.diag([-1.0 if flip_x else 1.0,
                                                                           -1.0 if flip_y else 1.0, 1.0]))
    A = A.astype(np.float32)
    inv = np.linalg.inv(A[:2, :2].astype(np.float64))
    D = np.diag([cell, cell])
    lo = np.array([-X * cell / 2, -Y * cell / 2])
    M = np.linalg.inv(D) @ inv @ D
    b = np.linalg.inv(D) @ (inv @ lo - lo)
    return np.concatenate([M, b[:, None]], axis=1).astype(np.float32), A


MATS = {"null": None, "identity": (0.0, 1.0, False, False), "rot30": (30.0, 0.9, True, False),
        "rot90": (90.0, 1.0, False, False)}


# ----------------------------------------------------------------------------- the restatement
def in_grid_ref(mats, X, Y):
    """k_class_masks_warp's range test: (n, X, Y) bool from (n, 2, 3) float32 matrices."""
    mats = np.asarray(mats)
    assert mats.dtype == np.float32 and mats.shape[1:] == (2, 3)
    half = np.float32(0.5)
    ci = (np.arange(X, dtype=np.float32) + half)[:, None]
    cj = (np.arange(Y, dtype=np.float32) + half)[None, :]
    out = np.empty((len(mats), X, Y), dtype=bool)
    for b, m in enumerate(mats):
        su = (m[0, 0] * ci + m[0, 1] * cj) + m[0, 2]
        sv = (m[1, 0] * ci + m[1, 1] * cj) + m[1, 2]
        assert su.dtype == np.float32 and sv.dtype == np.float32
        with np.errstate(invalid="ignore"):
            out[b] = (su >= 0) & (su < np.float32(X)) & (sv >= 0) & (sv < np.float32(Y))
    return out


def seen_ref(cam, qq, x, y, z, d_lo, d_hi, final_dim):
    """One camera's test on float32 points (arrays x, y; z an array or a scalar): the kernel's operations in order."""
    f = np.float32
    u_max, v_max = f(final_dim[1] - 1), f(final_dim[0] - 1)
    with np.errstate(all="ignore"):
        c = [((cam[3 * r] * x + cam[3 * r + 1] * y) + cam[3 * r + 2] * z) + cam[9 + r] for r in range(3)]
        d = c[2]
        up, vp = c[0] / d, c[1] / d
        u = (cam[12] * up + cam[13] * vp) + qq[0]
        v = (cam[14] * up + cam[15] * vp) + qq[1]
        assert u.dtype == np.float32 and v.dtype == np.float32 and d.dtype == np.float32
        return (d >= f(d_lo)) & (d < f(d_hi)) & (u >= 0) & (u <= u_max) & (v >= 0) & (v <= v_max)


def valid_mask_ref(cams, q, X, Y, x0, dx, y0, dy, heights, d_lo, d_hi, final_dim, mats=None, mode="fov"):
    """lss_simbev_valid_mask: cams (n, N, 16) float32, q (n, N, 2) float32, x0 / dx / y0 / dy float32 -> (n, X, Y) uint8."""
    f = np.float32
    assert all(isinstance(v, np.float32) for v in (x0, dx, y0, dy))
    n = len(cams) if cams is not None else len(mats)
    ok = np.ones((n, X, Y), dtype=bool) if mats is None else in_grid_ref(mats, X, Y)
    if mode == "grid":
        return ok.astype(np.uint8)
    cams, q = np.asarray(cams), np.asarray(q)
    assert cams.dtype == np.float32 and q.dtype == np.float32 and cams.shape[2] == 16 and q.shape[2] == 2
    x = (x0 + np.arange(X, dtype=np.float32) * dx)[:, None] + np.zeros((1, Y), dtype=np.float32)
    y = (y0 + np.arange(Y, dtype=np.float32) * dy)[None, :] + np.zeros((X, 1), dtype=np.float32)
    assert x.dtype == np.float32 and y.dtype == np.float32
    seen = np.zeros((n, X, Y), dtype=bool)
    for b in range(n):
        for z in heights:
            for cam, qq in zip(cams[b], q[b]):
                seen[b] |= seen_ref(cam, qq, x, y, f(z), d_lo, d_hi, final_dim)
    return (ok & seen).astype(np.uint8)


def case(grid, n, N, heights="one", mats="null", mode="fov"):
    """One case's inputs and reference: dict with the float32 cams / q (from the float64 construction, rounded once),
    the grid's arguments, the index matrices (or None) and `want`. The rig is composed with the matrices' A, as the
    loader composes it."""
    X, Y, cell = GRIDS[grid]
    rig = golden_rig(n, N)
    m = None
    if MATS[mats] is not None:
        pairs = [index_matrix(*MATS[mats], X, Y, cell) for _ in range(n)]
        m = np.stack([p[0] for p in pairs])
        rig = compose(rig, np.stack([p[1] for p in pairs]))
    cams, q = cameras64(rig)
    cams, q = cams.astype(np.float32), q.astype(np.float32)
    x0, dx, y0, dy = grid_args(X, Y, cell)
    want = valid_mask_ref(cams, q, X, Y, x0, dx, y0, dy, HEIGHTS[heights], DBOUND[0], DBOUND[1], FINAL_DIM, m, mode)
    return {"X": X, "Y": Y, "cell": cell, "rig": rig, "cams": cams, "q": q, "mats": m, "want": want,
            "heights": HEIGHTS[heights], "grid_conf": grid_conf(X, Y, cell)}


def gpu_cases():
    """(grid, n, N, heights, mats) of every fov-mode GPU case."""
    return [(g, n, N, h, m) for g in GPU_GRIDS for n, N in ((1, 6), (3, 1), (3, 6), (1, 1)) for h in HEIGHTS
            for m in MATS]


# ----------------------------------------------------------------------------- the masked loss, restated
def masked_closed_form(x, t, valid, rows):
    """(loss, d loss / dx) of the masked loss from the definition, in x's dtype (float64 for the reference): the focal
    term of tests/focal_cases.py per element, elements of cells with valid == 0 selected out, the sum over
    max(M, 1), M the number of valid elements. x, t (B, K, X, Y) torch tensors, valid (B, X, Y), rows K x 3."""
    import torch

    from focal_cases import softplus
    r = torch.as_tensor(rows, dtype=x.dtype).view(-1, 1, 1, 3)
    wp, wn, g = r[..., 0], r[..., 1], r[..., 2]
    q = t != 0
    p, pm = torch.sigmoid(x), torch.sigmoid(-x)
    l1 = torch.exp(-g * softplus(x)) * wp * softplus(-x)
    g1 = -torch.exp(-g * softplus(x)) * wp * (g * p * softplus(-x) + pm)
    l0 = torch.exp(-g * softplus(-x)) * wn * softplus(x)
    g0 = torch.exp(-g * softplus(-x)) * wn * (g * pm * softplus(x) + p)
    on = (valid != 0).unsqueeze(1).expand_as(x)
    m = max(int(on.sum()), 1)
    zero = torch.zeros((), dtype=x.dtype)
    return torch.where(on, torch.where(q, l1, l0), zero).sum() / m, torch.where(on, torch.where(q, g1, g0), zero) / m
