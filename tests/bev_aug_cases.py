"""What the BEV-space augmentation tests share: the label warp of lss_simbev_class_masks_warp restated in numpy,
independently of the package -- float32 arrays, the kernel's operation order (numpy rounds every product and sum
once and fuses nothing), np.floor, the same range test on the floats and the same flipud -- plus the data and the
matrices of the cases."""
import numpy as np

GC = {"xbound": [-50.0, 50.0, 0.5], "ybound": [-50.0, 50.0, 0.5], "zbound": [-10.0, 10.0, 20.0],
      "dbound": [4.0, 45.0, 1.0]}
DAC = {"resize_lim": (1.6, 1.8), "final_dim": (64, 192), "rot_lim": (-5.4, 5.4), "H": 56, "W": 120,
       "rand_flip": True, "bot_pct_lim": (0.0, 0.22), "Ncams": 6}
BEV_ON = {"bev_rot_lim": (-22.5, 22.5), "bev_scale_lim": (0.9, 1.1), "bev_flip": True}
BEV_NEUTRAL = {"bev_rot_lim": (0.0, 0.0), "bev_scale_lim": (1.0, 1.0), "bev_flip": False}
VEHICLE = [[1, 2, 3]]
THREE = [[0], [1, 2, 3], [6, 7]]
# (theta_deg, flip_x, flip_y) at scale 1 -> what the warped label is, as a function of the un-warped (X, Y) label
# in the (x rows, y columns) layout
SYMMETRIES = {
    "rot90": ((90.0, False, False), lambda a: np.rot90(a, 1)),
    "rot180": ((180.0, False, False), lambda a: a[::-1, ::-1]),
    "rot270": ((270.0, False, False), lambda a: np.rot90(a, 3)),
    "flip_x": ((0.0, True, False), lambda a: a[::-1, :]),
    "flip_y": ((0.0, False, True), lambda a: a[:, ::-1]),
    "flip_xy": ((0.0, True, True), lambda a: a[::-1, ::-1]),
}
SQUARE_ONLY = ("rot90", "rot270")


def grid_conf(X, Y, cell=0.5):
    """A grid of X x Y cells of `cell` metres centred on the ego."""
    return {"xbound": [-X * cell / 2, X * cell / 2, cell], "ybound": [-Y * cell / 2, Y * cell / 2, cell],
            "zbound": [-10.0, 10.0, 20.0], "dbound": [4.0, 45.0, 1.0]}


def bev_maps(n, C, X, Y, seed, density=0.3):
    """(n, C, X, Y) uint8, about `density` of the cells of every channel set, to any value > 0."""
    rng = np.random.default_rng(seed)
    return ((rng.random((n, C, X, Y)) < density) * rng.integers(1, 256, (n, C, X, Y))).astype(np.uint8)


def plain_labels(bev, groups):
    """lss_simbev_class_masks: flipud of each group's merge, (n, K, X, Y) float32."""
    return np.stack([np.flip(np.any(bev[:, g] > 0, axis=1), axis=1) for g in groups], axis=1).astype(np.float32)


def warp_labels(bev, groups, mats):
    """lss_simbev_class_masks_warp: bev (n, C, X, Y) uint8, mats (n, 2, 3) float32 -> (n, K, X, Y) float32."""
    n, _, X, Y = bev.shape
    mats = np.asarray(mats)
    assert mats.dtype == np.float32 and mats.shape == (n, 2, 3)
    src = plain_labels(bev, groups)  # src[b, k, si, sj] = any(bev[b, c, X-1-si, sj] > 0)
    half = np.float32(0.5)
    ci = (np.arange(X, dtype=np.float32) + half)[:, None]
    cj = (np.arange(Y, dtype=np.float32) + half)[None, :]
    out = np.empty_like(src)
    for b in range(n):
        m = mats[b]
        su = (m[0, 0] * ci + m[0, 1] * cj) + m[0, 2]
        sv = (m[1, 0] * ci + m[1, 1] * cj) + m[1, 2]
        assert su.dtype == np.float32 and sv.dtype == np.float32
        with np.errstate(invalid="ignore"):
            inside = (su >= 0) & (su < np.float32(X)) & (sv >= 0) & (sv < np.float32(Y))
        si = np.where(inside, np.floor(su), 0).astype(np.int64)
        sj = np.where(inside, np.floor(sv), 0).astype(np.int64)
        out[b] = np.where(inside[None], src[b][:, si, sj], np.float32(0))
    return out
