"""What the learning-rate schedule and the EMA cost in graph B (the captured update), at config 3's parameter count.

The flat masters of the c3 model exactly as the trainer groups them (three tensors, 14.3 M fp32), random gradients,
the update alone captured into one HIP graph and replayed; four variants, each in a fresh process, alternating:

  a  today's guarded update                      lss_clip_adam_guarded
  b  the new entry with a cosine schedule        lss_clip_adam_sched, ema = NULL
  c  a schedule and the EMA                      lss_clip_adam_sched, 36 B per parameter
  d  what a user could assemble before           a, then torch._foreach_lerp_ over the masters in the same graph

    python scripts/measure.py --tag r11 "py:sched_ema_bench:sched_ema_bench.py --rounds 3"

prints one line per run and a summary (median of each variant's runs, its spread), then the same as one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

VARIANTS = ("a", "b", "c", "d")


def child(variant: str, replays: int, reps: int) -> dict:
    import torch

    import lss_carla_amd as L
    from lss_carla_amd import optim, parallel, synthetic as syn
    from lss_carla_amd.flat_params import FlatParamGroups, lss_backward_groups

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    _, gc, dac = syn.config_confs("c3")
    model = L.compile_model(gc, dac, outC=1).to(dev)
    parallel.freeze_unused(model)
    flat = FlatParamGroups(model, lss_backward_groups(), cast_dtype=torch.bfloat16)
    masters = flat.masters
    for m in masters:
        m.grad = torch.randn_like(m) * 1e-2
    opt = torch.optim.Adam(masters, lr=1e-3, weight_decay=1e-7, fused=True, capturable=True)
    assert optim.supported(opt, masters)
    skipped = torch.zeros(1, device=dev, dtype=torch.int32)
    emas = flat.enable_ema() if variant in ("c", "d") else None
    sched = optim.LRSchedule("cosine", warmup_steps=100, warmup_factor=0.1, total_steps=100000, min_factor=0.01)
    if variant == "a" or variant == "d":
        ca = optim.ClipAdam(opt)
    elif variant == "b":
        ca = optim.ClipAdam(opt, schedule=sched)
    else:
        ca = optim.ClipAdam(opt, schedule=sched, ema=emas, ema_decay=0.999)

    def update():
        ca.step(5.0, skipped=skipped)
        if variant == "d":
            torch._foreach_lerp_(emas, [m.detach() for m in masters], 1.0 - 0.999)

    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        update()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        update()
    for _ in range(50):
        graph.replay()
    torch.cuda.synchronize(dev)
    times = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(replays):
            graph.replay()
        t1.record()
        torch.cuda.synchronize(dev)
        times.append(t0.elapsed_time(t1) * 1e3 / replays)
    assert skipped.item() == 0 and all(torch.isfinite(m).all() for m in masters)
    numel = sum(m.numel() for m in masters)
    return {"variant": variant, "us_per_replay": statistics.median(times), "min": min(times), "max": max(times),
            "numel": numel, "tensors": len(masters)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=VARIANTS, default=None, help="(child) measure one variant in this process")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if a.only:
        print(json.dumps(child(a.only, a.replays, a.reps)), flush=True)
        return
    runs = {v: [] for v in VARIANTS}
    for r in range(a.rounds):
        for v in VARIANTS:  # alternating: one fresh process per variant and round
            out = subprocess.run(["timeout", "-k", "10", "150", sys.executable, "-u", os.path.abspath(__file__), "--only", v,
                                  "--replays", str(a.replays), "--reps", str(a.reps)], capture_output=True, text=True)
            last = (out.stdout.strip().splitlines() or [""])[-1]
            if out.returncode != 0 or not last.startswith("{"):
                print(out.stdout[-2000:], out.stderr[-4000:], flush=True)
                sys.exit(out.returncode or 1)  # nothing more is started after a failure
            got = json.loads(last)
            runs[v].append(got)
            print(f"round {r} {v}: {got['us_per_replay']:8.2f} us / replay  (min {got['min']:.2f}, max {got['max']:.2f}; "
                  f"{got['numel']} parameters in {got['tensors']} tensors)", flush=True)
    names = {"a": "guarded update (today)", "b": "sched entry, cosine", "c": "sched entry, cosine + EMA",
             "d": "guarded update + torch._foreach_lerp_"}
    summary = {}
    print(f"# graph B alone, {a.replays} replays x {a.reps} timings per process, {a.rounds} fresh processes each, alternating")
    for v in VARIANTS:
        med = [g["us_per_replay"] for g in runs[v]]
        summary[v] = {"median_us": statistics.median(med), "runs_us": med}
        print(f"{v}  {names[v]:40s} {statistics.median(med):8.2f} us   runs {' '.join('%.2f' % m for m in med)}")
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
