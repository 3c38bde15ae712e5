"""Graph-replay times of the exclusive-class loss and metrics on (8, C, 200, 200) bf16 logits (config-3's BEV map) with
an (8, 200, 200) uint8 class map (3 % of the labels 255) and a valid-cell mask about 70 % set, for C = 4 and 8:

  loss forward + backward   tools.SoftmaxLoss on lss_softmax_ce (+ lss_seg_loss_masked_bwd) against
                            F.cross_entropy(weight=, ignore_index=255) on the fp32 cast of the logits, the mask folded
                            into the labels beforehand (outside the timed graph: torch's side is given that for free)
  validation accumulate     tools.confusion_accumulate on lss_confusion_accum against argmax + a bincount of
                            label * C + pred into a C x C matrix (written as scatter_add_ of ones: torch.bincount reads
                            its output size back to the host and cannot be captured) plus the same F.cross_entropy for
                            the loss term

  python scripts/softmax_bench.py [--classes 4 8] [--replays 50] [--rounds 5]

Each variant is captured once (torch.cuda.CUDAGraph, after eager warm-up) and timed with device events around
`replays` back-to-back replays, `rounds` times, the variants taking turns; the table gives the median and the range
of the per-replay time, and says whether every HIP run beat every torch run. One JSON line at the end."""
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
    ap.add_argument("--classes", type=int, nargs="+", default=[4, 8])
    ap.add_argument("--shape", type=int, nargs=3, default=[8, 200, 200], help="N H W")
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from lss_carla_amd import tools as T

    if not torch.cuda.is_available():
        raise SystemExit("softmax_bench: needs an MI355X")
    dev = torch.device("cuda:0")
    N, H, W = a.shape
    out = {"shape": [N, H, W], "replays": a.replays, "rounds": a.rounds, "unit": "us per graph replay"}
    for C in a.classes:
        torch.manual_seed(C)
        logits = torch.randn(N, C, H, W, device=dev).bfloat16().requires_grad_(True)
        labels = torch.randint(0, C, (N, H, W), device=dev).to(torch.uint8)
        labels[torch.rand(N, H, W, device=dev) < 0.03] = 255
        valid = (torch.rand(N, H, W, device=dev) < 0.7).to(torch.uint8)
        weights = [1.0 + 0.25 * c for c in range(C)]
        fn = T.SoftmaxLoss(C, weights).to(dev)
        w = fn.class_weight
        folded = torch.where(valid != 0, labels, torch.full_like(labels, 255)).long()  # torch's labels, mask applied
        totals = torch.zeros(1 + C * C, device=dev, dtype=torch.float64)
        conf = torch.zeros(C * C + 1, device=dev, dtype=torch.float64)  # (the last bin: cells that do not count)
        ones = torch.ones(N * H * W, device=dev, dtype=torch.float64)
        loss_sum = torch.zeros((), device=dev, dtype=torch.float64)

        def torch_metrics():
            x = logits.detach().float()
            pred = x.argmax(dim=1)
            on = folded != 255
            idx = torch.where(on, folded * C + pred, torch.full_like(folded, C * C))
            conf.scatter_add_(0, idx.reshape(-1), ones)
            loss_sum.add_(F.cross_entropy(x, folded, weight=w, ignore_index=255).double() * N)

        grads = {"softmax_hip_fwd_bwd": lambda: fn(logits, labels, valid),
                 "softmax_torch_fwd_bwd": lambda: F.cross_entropy(logits.float(), folded, weight=w, ignore_index=255)}
        plain = {"confusion_hip": lambda: T.confusion_accumulate(logits, labels, totals, None, w, valid=valid),
                 "confusion_torch": torch_metrics}
        graphs = {}
        for key, f in {**grads, **plain}.items():
            run = (lambda f=f: torch.autograd.grad(f(), logits)) if key in grads else f
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side), torch.set_grad_enabled(key in grads):
                for _ in range(3):
                    run()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g), torch.set_grad_enabled(key in grads):
                keep = run()
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
        print(f"C = {C}   {'variant':24s} {'median':>9s} {'min':>9s} {'max':>9s}   (us per replay; {a.rounds} x "
              f"{a.replays} replays)")
        res = {}
        for key, v in times.items():
            res[key] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
            print(f"        {key:24s} {res[key]['median']:9.1f} {min(v):9.1f} {max(v):9.1f}")
        res["softmax_hip_beats_every_torch_run"] = max(times["softmax_hip_fwd_bwd"]) < min(times["softmax_torch_fwd_bwd"])
        res["confusion_hip_beats_every_torch_run"] = max(times["confusion_hip"]) < min(times["confusion_torch"])
        print(f"        every HIP loss run beat every torch run: {res['softmax_hip_beats_every_torch_run']}; "
              f"confusion: {res['confusion_hip_beats_every_torch_run']}")
        out[f"C{C}"] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
