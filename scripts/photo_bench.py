"""Kernel time of the image augmentation with and without the photometric work (scripts/measure.py's photo step):
lss_simbev_images against lss_simbev_images_photo at the staging shape of config 3 -- 48 images (B = 8, N = 6) of
224 x 480 -> 128 x 352 -- under one seeded augmentation draw per sample (resize, crop, flip, rotation), with
neutral records, colour only, and colour + noise. Each variant is a HIP graph of --launches launches, replayed
--replays times between two device events; the variants alternate over --rounds rounds and the median of the rounds is
reported. With --parent-lib, the plain kernel of that library (the parent commit's build) is one more variant: the
comparison base. One JSON line: {"us_per_launch": {variant: median}, "rounds": {variant: [...]}, ...}.

  python scripts/photo_bench.py [--parent-lib PATH/liblss_hip.so]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    import numpy as np
    import torch
    from lss_carla_amd import _lib, simbev
    if not torch.cuda.is_available():
        raise SystemExit("photo_bench: needs an MI355X")
    dev = torch.device("cuda:0")
    B, N, H, W, fd = 8, 6, 224, 480, (128, 352)
    conf = {"H": H, "W": W, "final_dim": fd, "resize_lim": (0.8, 1.0), "bot_pct_lim": (0.0, 0.22),
            "rot_lim": (-5.4, 5.4), "rand_flip": True}
    np.random.seed(0)
    augs = []
    for _ in range(B):
        _, rd, crop, flip, rot = simbev.draw_augmentation(conf, True)
        augs.extend([{"resize_dims": rd, "crop": crop, "flip": flip, "rotate": rot}] * N)
    n = B * N
    src = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (n, H, W, 3), dtype=np.uint8)).to(dev)
    records = {
        "photo_neutral": np.stack([simbev.photo_record()] * n),
        "photo_colour": np.stack([simbev.photo_record(20.0 - i, 0.7 + 0.01 * i, 1.3 - 0.01 * i, i - 18.0) for i in range(n)]),
        "photo_colour_noise": np.stack([simbev.photo_record(20.0 - i, 0.7 + 0.01 * i, 1.3 - 0.01 * i, i - 18.0, 8.0, i, 1)
                                        for i in range(n)]),
    }
    keep: list = []
    out = torch.empty(n, 3, *fd, device=dev)
    plain = simbev.augment_images(src, augs, fd, keep=keep).clone()
    par_d, tab_d = keep[0], keep[1]
    photo_d = {k: torch.from_numpy(v).to(dev) for k, v in records.items()}
    neutral = simbev.augment_images(src, augs, fd, photo=torch.from_numpy(records["photo_neutral"]))
    assert torch.equal(plain, neutral), "neutral records differ from the plain kernel"
    lib = _lib.load()
    p = _lib.ptr
    variants = {"plain": lambda st: lib.lss_simbev_images(p(src), n, H, W, p(par_d), p(tab_d), fd[0], fd[1], p(out), st)}
    if a.parent_lib:
        parent = ctypes.CDLL(a.parent_lib)
        parent.lss_simbev_images.restype = ctypes.c_int
        parent.lss_simbev_images.argtypes = lib.lss_simbev_images.argtypes
        parent.lss_abi_version.restype = ctypes.c_int
        variants["parent_plain"] = lambda st: parent.lss_simbev_images(p(src), n, H, W, p(par_d), p(tab_d), fd[0], fd[1],
                                                                       p(out), st)
    for name, rec in photo_d.items():
        variants[name] = (lambda rec: lambda st: lib.lss_simbev_images_photo(p(src), n, H, W, p(par_d), p(rec), p(tab_d),
                                                                             fd[0], fd[1], p(out), st))(rec)
    graphs = {}
    for name, launch in variants.items():
        assert launch(_lib.stream_handle(dev)) == 0, name  # warm-up: the code object is loaded
        torch.cuda.synchronize()
        if name in ("plain", "parent_plain"):
            assert torch.equal(out, plain), name
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(a.launches):
                assert launch(_lib.stream_handle(dev)) == 0, name
        g.replay()
        graphs[name] = g
    torch.cuda.synchronize()
    rounds = {k: [] for k in graphs}
    for _ in range(a.rounds):
        for name, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.replays):
                g.replay()
            e1.record()
            e1.synchronize()
            rounds[name].append(e0.elapsed_time(e1) * 1e3 / (a.replays * a.launches))
    out_bytes = n * 3 * fd[0] * fd[1] * 4
    print(json.dumps({"shape": {"images": n, "src": [H, W], "final_dim": list(fd)}, "launches_per_graph": a.launches,
                      "replays_per_round": a.replays, "out_bytes": out_bytes, "src_bytes": n * H * W * 3,
                      "us_per_launch": {k: round(statistics.median(v), 2) for k, v in rounds.items()},
                      "rounds": {k: [round(x, 2) for x in v] for k, v in rounds.items()},
                      "parent_abi": parent.lss_abi_version() if a.parent_lib else None}))


if __name__ == "__main__":
    main()
