"""Frames/s of trainer.train's steps on a synthetic SimBEV tree at config-3 sizes (scripts/measure.py's
train_loop step): one JSON line {"frames_per_s", "steps", "nworkers", "cycle_batches", ...}.

  python scripts/train_loop.py --dataroot DIR --steps 200 --nworkers 14            the loop as a user runs it
  python scripts/train_loop.py --dataroot DIR --steps 200 --cycle-batches 4        pre-decoded host batches cycled:
                                                                                    the step plus the staging only
  python scripts/train_loop.py --make DIR --samples 2000                           write the tree and exit
  python scripts/train_loop.py --dataroot DIR --label-groups "0;1,2;3"             a multi-class run (on a tree made
                                                                                    with --box-classes 0,1,2,3)
  python scripts/train_loop.py --dataroot DIR --loss focal [--focal-gamma 2.0]     the focal loss (--pos-weight its w_pos)
  python scripts/train_loop.py --dataroot DIR --bev-rot-lim=-22.5,22.5 --bev-scale-lim 0.9,1.1 --bev-flip 1
                                                                                    the BEV-space augmentation
  python scripts/train_loop.py --dataroot DIR --valid-mask fov [--fov-z 0.0,1.5]   the valid-cell mask (none | grid | fov)
  python scripts/train_loop.py --dataroot DIR --label-groups "0;1,2;3" --exclusive 1 [--class-weight 1,1,2,4]
                                                                                    exclusive classes (softmax loss)
  python scripts/train_loop.py --dataroot DIR --photo 1                            the photometric augmentation, every
                                                                                    op on (+-32, 0.5-1.5, 0.5-1.5, +-18 deg,
                                                                                    sigma 0-8, per camera)
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--make", default="")
    ap.add_argument("--samples", type=int, default=2000, help="--make: samples written (80 % are the training split)")
    ap.add_argument("--dataroot", default="")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--bsz", type=int, default=8)
    ap.add_argument("--nworkers", type=int, default=14)
    ap.add_argument("--cycle-batches", type=int, default=0)
    ap.add_argument("--graph", type=int, default=1)
    ap.add_argument("--miopen-find", type=int, default=0)
    ap.add_argument("--label-groups", default="", help='trainer --label_groups, e.g. "0;1,2;3" (default: the vehicle mask)')
    ap.add_argument("--pos-weight", default="2.13", help="trainer --pos_weight: one weight, or one per class")
    ap.add_argument("--loss", default="bce", choices=["bce", "focal"], help="trainer --loss")
    ap.add_argument("--focal-gamma", default="2.0", help="trainer --focal_gamma")
    ap.add_argument("--box-classes", default="1,2,3", help="--make: the BEV channels the boxes are drawn in")
    ap.add_argument("--bev-rot-lim", default="0,0", help="trainer --bev_rot_lim")
    ap.add_argument("--bev-scale-lim", default="1,1", help="trainer --bev_scale_lim")
    ap.add_argument("--bev-flip", type=int, default=0, help="trainer --bev_flip")
    ap.add_argument("--valid-mask", default="none", choices=["none", "grid", "fov"], help="trainer --valid_mask")
    ap.add_argument("--fov-z", default="0.0", help="trainer --fov_z")
    ap.add_argument("--ncams", type=int, default=6, help="trainer --ncams: cameras per training sample")
    ap.add_argument("--exclusive", type=int, default=0, help="trainer --exclusive (needs --label-groups)")
    ap.add_argument("--class-weight", default="", help="trainer --class_weight: one weight per class, background first")
    ap.add_argument("--photo", type=int, default=0, help="1: trainer --photo_brightness 32 --photo_contrast 0.5,1.5 "
                    "--photo_saturation 0.5,1.5 --photo_hue 18 --photo_noise 0,8")
    a = ap.parse_args()
    from lss_carla_amd import miopen_db
    miopen_db.use_committed()  # before torch starts
    from lss_carla_amd import synthetic as syn
    if a.make:
        per_scene = 20
        n = syn.make_simbev_tree(a.make, (a.samples + per_scene - 1) // per_scene, per_scene,
                                 box_classes=tuple(int(c) for c in a.box_classes.split(",")))
        print(json.dumps({"made": a.make, "samples": n}))
        return
    from lss_carla_amd import trainer
    with tempfile.TemporaryDirectory() as logdir:
        out = trainer.train(a.dataroot, nepochs=1000, bsz=a.bsz, nworkers=a.nworkers, logdir=logdir,
                            val_step=10 ** 9, save_step=10 ** 9, use_wandb=False, graph=bool(a.graph),
                            miopen_find=bool(a.miopen_find), seed=0, max_steps=a.steps,
                            cycle_batches=a.cycle_batches, label_groups=trainer.parse_label_groups(a.label_groups),
                            pos_weight=None if a.exclusive else trainer.parse_pos_weight(a.pos_weight), loss=a.loss,
                            focal_gamma=trainer.parse_per_class(a.focal_gamma, "--focal-gamma"),
                            bev_rot_lim=trainer.parse_pair(a.bev_rot_lim, "--bev-rot-lim"),
                            bev_scale_lim=trainer.parse_pair(a.bev_scale_lim, "--bev-scale-lim"),
                            bev_flip=bool(a.bev_flip), valid_mask=a.valid_mask,
                            fov_z=trainer.parse_heights(a.fov_z), ncams=a.ncams,
                            **({"photo_brightness": 32.0, "photo_contrast": (0.5, 1.5), "photo_saturation": (0.5, 1.5),
                                "photo_hue": 18.0, "photo_noise": (0.0, 8.0)} if a.photo else {}),
                            **({"exclusive": True, "class_weight": [float(v) for v in a.class_weight.split(",")]
                                if a.class_weight else None} if a.exclusive else {}))
    print(json.dumps({"frames_per_s": out["frames_per_s"], "steps": out["counter"], "bsz": a.bsz,
                      "nworkers": a.nworkers, "cycle_batches": a.cycle_batches, "graph": a.graph,
                      "skipped": out["skipped"], "loss": out["loss"], "label_groups": a.label_groups or None,
                      "loss_kind": a.loss, "bev_rot_lim": a.bev_rot_lim, "bev_scale_lim": a.bev_scale_lim,
                      "bev_flip": a.bev_flip, "valid_mask": a.valid_mask, "fov_z": a.fov_z, "ncams": a.ncams,
                      "exclusive": a.exclusive, "photo": a.photo}))


if __name__ == "__main__":
    main()
