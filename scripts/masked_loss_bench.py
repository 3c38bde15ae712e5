"""Graph-replay times of the masked loss, forward + backward, on (8, K, 200, 200) bf16 logits (config-3's BEV map) with
a (8, 200, 200) uint8 valid-cell mask about 70 % set: tools.FocalLoss with valid= on lss_seg_loss_masked, the same
module without the mask on lss_focal_logits_pc, and the masked formula composed from torch ops (what a user would
write without the kernel: the focal terms, torch.where, the division by the valid count), in one process, alternating.

  python scripts/masked_loss_bench.py [--K 8] [--gamma 2.0] [--replays 50] [--rounds 5]

Each variant is captured once (torch.cuda.CUDAGraph, after eager warm-up) and timed with device events around
`replays` back-to-back replays, `rounds` times, the variants taking turns; the table gives the median and the
range of the per-replay time. One JSON line at the end."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=8)
    ap.add_argument("--shape", type=int, nargs=3, default=[8, 200, 200], help="N H W")
    ap.add_argument("--gamma", type=float, default=2.0)
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from lss_carla_amd import tools as T

    if not torch.cuda.is_available():
        raise SystemExit("masked_loss_bench: needs an MI355X")
    dev = torch.device("cuda:0")
    N, H, W = a.shape
    K = a.K
    torch.manual_seed(0)
    logits = torch.randn(N, K, H, W, device=dev).bfloat16().requires_grad_(True)
    labels = (torch.rand(N, K, H, W, device=dev) < 0.03).float()
    valid = (torch.rand(N, H, W, device=dev) < 0.7).to(torch.uint8)
    weights = [1.0 + 0.5 * k for k in range(K)]
    focal = T.FocalLoss(K, gamma=a.gamma, pos_weight=weights).to(dev)
    pw = torch.tensor(weights, device=dev).view(K, 1, 1)

    def masked_torch(x, t, v):
        x = x.float()
        ce = F.binary_cross_entropy_with_logits(x, t, pos_weight=pw, reduction="none")
        p = torch.sigmoid(x)
        p_t = p * t + (1 - p) * (1 - t)
        on = (v != 0).unsqueeze(1).expand_as(x)
        terms = torch.where(on, (1 - p_t) ** a.gamma * ce, torch.zeros((), device=x.device))
        return terms.sum() / on.sum().clamp(min=1)

    variants = {"masked_hip_fwd_bwd": lambda: focal(logits, labels, valid),
                "focal_hip_fwd_bwd": lambda: focal(logits, labels),
                "masked_torch_fwd_bwd": lambda: masked_torch(logits, labels, valid)}
    graphs = {}
    for key, fn in variants.items():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                torch.autograd.grad(fn(), logits)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            keep = torch.autograd.grad(fn(), logits)
        graphs[key] = (g, keep)

    times = {k: [] for k in graphs}
    for _ in range(a.rounds):
        for key, (g, _) in graphs.items():
            g.replay()  # (the variant's working set back in the caches it will find when it repeats)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.replays):
                g.replay()
            t1.record()
            torch.cuda.synchronize()
            times[key].append(t0.elapsed_time(t1) * 1e3 / a.replays)  # us per replay
    out = {"shape": [N, K, H, W], "gamma": a.gamma, "valid_fraction": float(valid.float().mean()), "replays": a.replays,
           "rounds": a.rounds, "unit": "us per graph replay"}
    print(f"{'variant':24s} {'median':>9s} {'min':>9s} {'max':>9s}   (us per replay; {a.rounds} x {a.replays} replays)")
    for key, v in times.items():
        out[key] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
        print(f"{key:24s} {out[key]['median']:9.1f} {min(v):9.1f} {max(v):9.1f}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
