"""Graph-replay times of BevEncode's multi-class tail at config-3's shape: BN + ReLU + the 1x1 head to K
channels on a (8, 128, 200, 200) channels-last bf16 map, and the K-class loss on its (8, K, 200, 200) logits --
the HIP path (models._BnReluHeadK on lss_headk_*, SimpleLoss on lss_bce_logits_pc) against the generic path
(USE_HIP_HEADK off: bn_act + F.linear; torch's BCEWithLogitsLoss) in one process, alternating.

  python scripts/headk_bench.py [--K 8] [--replays 50] [--rounds 5]

Each variant is captured once (torch.cuda.CUDAGraph, after eager warm-up) and timed with device events
around `replays` back-to-back replays, `rounds` times, the variants taking turns; the table gives the median
and the range of the per-replay time. One JSON line at the end."""
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
    ap.add_argument("--shape", type=int, nargs=4, default=[8, 128, 200, 200])
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import torch
    from lss_carla_amd import models as M, tools as T

    if not torch.cuda.is_available():
        raise SystemExit("headk_bench: needs an MI355X")
    dev = torch.device("cuda:0")
    N, C, H, W = a.shape
    K = a.K
    torch.manual_seed(0)
    x = torch.randn(N, C, H, W, device=dev).bfloat16().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    bn = torch.nn.BatchNorm2d(C).to(dev).train()
    head = M.logits_head(torch.nn.Conv2d(C, K, 1).to(dev).to(memory_format=torch.channels_last))
    params = [x, bn.weight, bn.bias, head.weight, head.bias]
    logits = torch.randn(N, K, H, W, device=dev).bfloat16().requires_grad_(True)
    labels = (torch.rand(N, K, H, W, device=dev) < 0.03).float()
    weights = [1.0 + 0.5 * k for k in range(K)]
    loss_fn = T.SimpleLoss(weights).to(dev)

    def tail(hip, backward):
        M.USE_HIP_HEADK = hip
        with torch.autocast("cuda", dtype=torch.bfloat16, cache_enabled=False):
            if not backward:
                with torch.no_grad():
                    return M.bn_relu_head1(bn, head, x)
            y = M.bn_relu_head1(bn, head, x)
        dout = torch.ones_like(y)  # (the fallback's logits are channels-last: a gradient of its strides)
        return torch.autograd.grad(y, params, dout)

    def loss(hip, backward):
        if hip:
            val = loss_fn(logits, labels)
        else:  # what train_step does for a loss that does not compute in fp32 itself
            val = loss_fn.loss_fn(logits.float(), labels)
        return torch.autograd.grad(val, logits) if backward else val

    variants = {}
    for name, fn in (("tail", tail), ("loss", loss)):
        for hip in (True, False):
            for backward in (False, True):
                variants[f"{name}_{'hip' if hip else 'generic'}_{'fwd_bwd' if backward else 'fwd'}"] = (fn, hip, backward)

    graphs = {}
    for key, (fn, hip, backward) in variants.items():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                fn(hip, backward)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            keep = fn(hip, backward)
        graphs[key] = (g, keep)
    M.USE_HIP_HEADK = True

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
    out = {"shape": a.shape, "K": K, "replays": a.replays, "rounds": a.rounds, "unit": "us per graph replay"}
    print(f"{'variant':34s} {'median':>9s} {'min':>9s} {'max':>9s}   (us per replay; {a.rounds} x {a.replays} replays)")
    for key, v in times.items():
        out[key] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
        print(f"{key:34s} {out[key]['median']:9.1f} {min(v):9.1f} {max(v):9.1f}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
