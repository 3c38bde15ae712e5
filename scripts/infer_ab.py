"""The Predictor at config-3 sizes (6 x 128 x 352 images, D = 41, 200 x 200 BEV, bf16) with the eval-mode batch
norm kernels on and off (norm.USE_HIP_BN_EVAL), for scripts/measure.py's `infer` step.

  python scripts/infer_ab.py --bsz 8 --frames 400 --legs 3       A/B in one process: two Predictors (one captured
                                                                  with the switch on, one with it off, over copies
                                                                  of one model), their legs of graph replays
                                                                  alternating; one JSON line
  python scripts/infer_ab.py --bsz 8 --only on --calls 20        one switch only (under rocprofv3 --kernel-trace)
"""
from __future__ import annotations

import argparse
import copy
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

import lss_carla_amd as L  # noqa: E402
from lss_carla_amd import norm, synthetic as syn  # noqa: E402

RIG = ("rots", "trans", "intrins", "post_rots", "post_trans")


def build(bsz, dev, switch, model):
    norm.USE_HIP_BN_EVAL = switch
    p = L.Predictor(model, bsz, dev, amp_dtype=torch.bfloat16, graph=True)
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bsz", type=int, default=8)
    ap.add_argument("--frames", type=int, default=400, help="frames per leg (at least 200)")
    ap.add_argument("--legs", type=int, default=3)
    ap.add_argument("--only", default="", choices=["", "on", "off"])
    ap.add_argument("--calls", type=int, default=20, help="--only: replays")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.backends.cudnn.benchmark = not a.only  # (a traced run: no find-mode launches among the counted kernels)
    cfg, gc, dac = syn.config_confs("c3")
    B, N, fd = a.bsz, cfg["N"], cfg["final_dim"]
    torch.manual_seed(1234)
    model = L.compile_model(gc, dac, outC=1).to(dev)
    model.bevencode.to(memory_format=torch.channels_last)
    model.camencode.up1.to(memory_format=torch.channels_last)
    rig = syn.make_rig(B, N, fd, seed=0)
    # images and the device-side rig on the device, the two matrices HostInverses inverts on the host
    inputs = (syn.make_images(B, N, fd, seed=0).to(dev), rig["rots"].to(dev), rig["trans"].to(dev), rig["intrins"],
              rig["post_rots"], rig["post_trans"].to(dev))
    sides = [s for s in ("on", "off") if a.only in ("", s)]
    preds = {}
    for s in sides:
        preds[s] = build(B, dev, s == "on", copy.deepcopy(model))
        preds[s](*inputs)  # warm-up + capture, with this side's switch
    torch.cuda.synchronize()
    if a.only:
        for _ in range(a.calls):
            preds[a.only](*inputs)
        torch.cuda.synchronize()
        print(json.dumps({"only": a.only, "bsz": B, "replays": a.calls}))
        return
    calls = max(1, -(-max(a.frames, 200) // B))
    legs = {s: [] for s in sides}
    for _ in range(a.legs):
        for s in sides:
            p = preds[s]
            p(*inputs)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                p(*inputs)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            legs[s].append({"frames_per_s": round(calls * B / dt, 2), "ms_per_call": round(1e3 * dt / calls, 4)})
    diff = (preds["on"].logits().float() - preds["off"].logits().float()).abs().max().item()
    print(json.dumps({"bsz": B, "calls_per_leg": calls, "frames_per_leg": calls * B, "legs": legs,
                      "max_abs_logit_diff_on_vs_off": diff}))


if __name__ == "__main__":
    main()
