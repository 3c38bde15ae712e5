"""Camera-alive mask: what it costs. One process, graph replays, device events, variants alternating.

  plan       ops.plan_from_cameras at config 3 (B=8, N=6, D=41, 8x22, 200x200) captured alone: unmasked, masked with
             every camera alive, masked with one dead camera per sample
  predictor  Predictor bsz 8 at config-3 sizes, bf16: camera_mask off / on (all alive) / on (one dead per sample)

Prints one JSON line per measurement: median and range over --legs legs of --replays replays each, microseconds."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from lss_carla_amd import miopen_db  # noqa: E402

miopen_db.use_committed()  # before torch starts

import torch  # noqa: E402

import lss_carla_amd as L  # noqa: E402
from lss_carla_amd import ops, synthetic as syn  # noqa: E402


def timed(replay, replays):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(replays):
        replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / replays


def report(name, variants, legs, replays):
    for fn in variants.values():  # warm
        timed(fn, 10)
    got = {k: [] for k in variants}
    for _ in range(legs):
        for k, fn in variants.items():
            got[k].append(timed(fn, replays))
    for k, v in got.items():
        print(json.dumps({"what": name, "variant": k, "us_median": round(statistics.median(v), 2),
                          "us_min": round(min(v), 2), "us_max": round(max(v), 2), "legs": legs, "replays": replays}),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", type=int, default=5)
    ap.add_argument("--replays", type=int, default=200)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg, gc, dac = syn.config_confs("c3")
    B, N, fd = cfg["B"], cfg["N"], cfg["final_dim"]
    rig = {k: v.to(dev) for k, v in syn.make_rig(B, N, fd, seed=0).items()}
    model = L.compile_model(gc, dac, outC=1).to(dev)
    model.bevencode.to(memory_format=torch.channels_last)
    model.camencode.up1.to(memory_format=torch.channels_last)
    grid = ops.GridSpec.from_conf(gc)
    inv = ops.camera_inverses(rig["post_rots"], rig["intrins"])
    ones = torch.ones(B, N, device=dev, dtype=torch.uint8)
    one_dead = ones.clone()
    one_dead[torch.arange(B), torch.arange(B) % N] = 0

    def plan_graph(alive):
        def go():
            return ops.plan_from_cameras(model.frustum, **rig, grid=grid, inverses=inv, cam_alive=alive)
        go()  # the shape's workspace, outside capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            keep = go()
        return g, keep

    graphs = {"unmasked": plan_graph(None), "masked_all_alive": plan_graph(ones),
              "masked_one_dead_per_sample": plan_graph(one_dead)}
    report("plan_c3", {k: g.replay for k, (g, _) in graphs.items()}, a.legs, a.replays)
    del graphs

    host = syn.make_rig(B, N, fd, seed=0)
    inputs = (syn.make_images(B, N, fd, seed=0), *(host[k] for k in L.Predictor.RIG))
    # a model of its own per Predictor (each moves its module's parameters into its own flat master); same seed,
    # same weights

    def predictor(**kw):
        torch.manual_seed(0)
        m = L.compile_model(gc, dac, outC=1).to(dev)
        m.bevencode.to(memory_format=torch.channels_last)
        m.camencode.up1.to(memory_format=torch.channels_last)
        p = L.Predictor(m, B, dev, graph=True, **kw)
        p(*inputs)
        return p

    del model
    p_off, p_on = predictor(), predictor(camera_mask=True)
    variants = {"camera_mask_off": p_off.graph.replay, "camera_mask_on_all_alive": p_on.graph.replay}
    report("predictor_bsz8", variants, a.legs, max(a.replays // 4, 20))
    p_on.set_alive(one_dead)
    variants = {"camera_mask_on_one_dead_per_sample": p_on.graph.replay, "camera_mask_off": p_off.graph.replay}
    report("predictor_bsz8", variants, a.legs, max(a.replays // 4, 20))


if __name__ == "__main__":
    main()
