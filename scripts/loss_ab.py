"""Two builds of the library on the sigmoid-loss entries: every output bit compared, then graph-replay times.

  python scripts/loss_ab.py PARENT_LIB [--skip-times] [--replays 50] [--rounds 5]

PARENT_LIB is another build's liblss_hip.so (the parent commit's, built in a checkout of it); this tree's build is
_lib.LIB_PATH. Both are opened with _lib.open_library in one process and given the same device inputs.

Part 1 runs the ten entries of the sigmoid half of lss_loss.hip -- lss_bce_logits (+ _bwd), lss_bce_logits_pc,
lss_focal_logits_pc, lss_seg_loss_masked (+ _bwd), lss_bce_iou_accum, lss_bce_iou_accum_pc, lss_seg_metrics_accum,
lss_seg_metrics_accum_masked -- in fp32 and bf16 and compares every output buffer (loss, scale, stored gradient, dx,
totals, valid_cells) as raw bytes. Inputs: the shapes of tests/test_gpu_masked_loss.py and test_gpu_seg_metrics.py and
config 3's (8, K, 200, 200) with K = 1 and 8; plain logits and logits with +-inf, NaN and +-88 planted; hard and soft
labels; a ~70 % mask, an all-zero and an all-ones mask; n_valid 0, a middle value and the batch size; for the
accumulate entries also logits one element into a larger buffer. A case is one (shape, dtype, logits, labels): one
line for its 30 calls (every entry under every mask and n_valid); the first difference is printed with its call and
ends the run with exit status 1.

Part 2 times, at (8, 8, 200, 200) bf16, forward + backward of the four training losses and the four accumulates: each
captured once per library (torch.cuda.CUDAGraph) and timed with device events around `replays` back-to-back replays,
`rounds` times, the two libraries taking turns (scripts/masked_loss_bench.py's method). Both libraries read and write
the same buffers, so where a buffer lies in memory cannot favour one of them, and the one that goes first changes every
round. A row is "ok" when this tree's median is no higher than the
parent's slowest round; exit status 3 when a row is not. PARENT_LIB = a copy of this tree's build shows what the
method itself resolves."""
from __future__ import annotations

import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = [(3, 3, 5, 7), (2, 3, 20, 20), (2, 3, 19, 21), (3, 3, 5, 5), (3, 3, 50, 50), (2, 8, 16, 16), (2, 1, 200, 200),
          (8, 1, 200, 200), (8, 8, 200, 200)]
LADDER = [-0.62, -0.41, -0.2, 0.0, 0.2, 0.41, 0.62]  # logit thresholds, ascending
GOUT = 0.75


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent_lib")
    ap.add_argument("--skip-times", action="store_true")
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import torch
    from lss_carla_amd import _lib

    if not torch.cuda.is_available():
        raise SystemExit("loss_ab: needs an MI355X")
    dev = torch.device("cuda:0")
    libs = {"parent": _lib.open_library(os.path.abspath(a.parent_lib)), "this": _lib.open_library(_lib.LIB_PATH)}
    p, code = _lib.ptr, _lib.dtype_code
    stream = lambda: _lib.stream_handle(dev)  # noqa: E731
    f32 = dict(device=dev, dtype=torch.float32)
    gouts = torch.full((1,), GOUT, **f32)  # the incoming gradient of the loss

    def fresh(n, dtype):
        """an output buffer with a fixed pattern under whatever the entry leaves unwritten"""
        return torch.full((n,), 7, device=dev, dtype=torch.uint8).repeat(torch.empty((), dtype=dtype).element_size()).view(dtype)

    def ok(rc, what):
        if rc != 0:
            raise SystemExit(f"loss_ab: {what} returned {rc}")

    # ---- the entries, each returning its output buffers by name
    def train_bufs(lib, kind, x):
        n = x.numel()
        return {"partial": fresh((2 if kind == "masked" else 1) * int(lib.lss_bce_partials(n)), torch.float32),
                "loss": fresh(1, torch.float32), "scale": fresh(1, torch.float32), "grad": fresh(n, x.dtype),
                "dx": fresh(n, x.dtype)}

    def train(lib, kind, x, t, plane, K, w, valid=None, o=None):
        """kind: bce (w a float), pc (w the K weights), focal / masked (w the (K, 3) rows); then the backward"""
        n = x.numel()
        o = o or train_bufs(lib, kind, x)
        partial, loss, scale, grad, dx = o["partial"], o["loss"], o["scale"], o["grad"], o["dx"]
        head = (p(x), code(x.dtype), p(t))
        if kind == "bce":
            ok(lib.lss_bce_logits(*head, n, float(w), p(partial), p(loss), p(grad), stream()), "lss_bce_logits")
        elif kind == "pc":
            ok(lib.lss_bce_logits_pc(*head, n, plane, K, p(w), p(partial), p(loss), p(grad), stream()), "lss_bce_logits_pc")
        elif kind == "focal":
            ok(lib.lss_focal_logits_pc(*head, n, plane, K, p(w), p(partial), p(loss), p(grad), stream()),
               "lss_focal_logits_pc")
        else:
            ok(lib.lss_seg_loss_masked(*head, p(valid), n, plane, K, p(w), p(partial), p(loss), p(scale), p(grad), stream()),
               "lss_seg_loss_masked")
        if kind == "masked":
            ok(lib.lss_seg_loss_masked_bwd(p(grad), code(x.dtype), n, p(gouts), p(scale), p(dx), stream()),
               "lss_seg_loss_masked_bwd")
        else:
            ok(lib.lss_bce_logits_bwd(p(grad), code(x.dtype), n, p(gouts), p(dx), stream()), "lss_bce_logits_bwd")
        return o

    def accum_bufs(lib, kind, n, K):
        T = len(LADDER)
        nbytes = {"iou": lambda: lib.lss_bce_iou_partial_bytes(n), "iou_pc": lambda: lib.lss_bce_iou_pc_partial_bytes(n, K),
                  "seg": lambda: lib.lss_seg_metrics_partial_bytes(n, K, T),
                  "seg_masked": lambda: lib.lss_seg_metrics_masked_partial_bytes(n, K, T)}[kind]()
        nt = {"iou": 3, "iou_pc": 1 + 2 * K}.get(kind, 1 + K + 2 * K * T)
        return {"totals": torch.arange(nt, device=dev, dtype=torch.float64) * 0.5,  # accumulated into
                "valid_cells": torch.full((1,), 3.0, device=dev, dtype=torch.float64),
                "partial": fresh((int(nbytes) + 7) // 8, torch.float64)}

    def accum(lib, kind, x, t, batch, plane, K, w, n_valid, thetas=None, valid=None, o=None):
        """kind: iou (w a float), iou_pc (w the K weights), seg / seg_masked (w the rows, thetas the ladder)"""
        n, per, T = x.numel(), x.numel() // batch, len(LADDER)
        o = o or accum_bufs(lib, kind, n, K)
        totals, cells, partial = o["totals"], o["valid_cells"], o["partial"]
        head = (p(x), code(x.dtype), p(t))
        if kind == "iou":
            ok(lib.lss_bce_iou_accum(*head, per, batch, p(n_valid), float(w), p(totals), p(partial), stream()),
               "lss_bce_iou_accum")
        elif kind == "iou_pc":
            ok(lib.lss_bce_iou_accum_pc(*head, per, batch, p(n_valid), plane, K, p(w), p(totals), p(partial), stream()),
               "lss_bce_iou_accum_pc")
        elif kind == "seg":
            ok(lib.lss_seg_metrics_accum(*head, per, batch, p(n_valid), plane, K, p(w), p(thetas), T, p(totals), p(partial),
                                         stream()), "lss_seg_metrics_accum")
        else:
            ok(lib.lss_seg_metrics_accum_masked(*head, p(valid), per, batch, p(n_valid), plane, K, p(w), p(thetas), T,
                                                p(totals), p(cells), p(partial), stream()), "lss_seg_metrics_accum_masked")
        return o

    def same(what, fn):
        """fn(lib) on both libraries; every buffer as raw bytes"""
        outs = {side: fn(lib) for side, lib in libs.items()}
        torch.cuda.synchronize()
        for name, want in outs["parent"].items():
            got = outs["this"][name]
            if not torch.equal(want.view(torch.uint8), got.view(torch.uint8)):
                diff = (want.view(torch.uint8) != got.view(torch.uint8)).nonzero()
                print(f"{what}: {name} DIFFERS in {diff.numel()} bytes, the first at byte {int(diff[0])}: parent "
                      f"{want.view(-1)[int(diff[0]) // want.element_size()].item()!r} this "
                      f"{got.view(-1)[int(diff[0]) // got.element_size()].item()!r}", flush=True)
                raise SystemExit(1)
        return len(outs["parent"])

    # ---- part 1
    cases = calls = 0
    thetas = torch.tensor(LADDER, **f32)
    for shape in SHAPES:
        B, K = shape[:2]
        plane, n = shape[2] * shape[3], B * K * shape[2] * shape[3]
        g = torch.Generator().manual_seed(1000 * n + K)
        pw = 2.13
        pwc = torch.tensor([0.5 + 0.75 * k for k in range(K)], **f32)
        rows = torch.tensor([(0.25 + 0.5 * k / K, 1.0 - 0.3 * k / K, (0.0, 2.0, 0.5)[k % 3]) for k in range(K)], **f32)
        masks = {"mask70": (torch.rand(B, plane, generator=g) < 0.7).to(torch.uint8).to(dev),
                 "mask0": torch.zeros(B, plane, device=dev, dtype=torch.uint8),
                 "mask1": torch.ones(B, plane, device=dev, dtype=torch.uint8)}
        for logits in ("plain", "special"):
            x32 = torch.randn(n, generator=g) * 3
            if logits == "special":  # planted over the whole range, the last elements included
                at = torch.randperm(n, generator=g)[:max(6, n // 50)]
                at[:6] = torch.tensor([0, 1, n - 1, n - 2, n // 2, n // 3])
                x32[at] = torch.tensor([float("inf"), float("-inf"), float("nan"), 88.0, -88.0, 0.0])[torch.arange(at.numel()) % 6]
            for labels in ("hard", "soft"):
                t = ((torch.rand(n, generator=g) < 0.3).float() if labels == "hard" else torch.rand(n, generator=g)).to(dev)
                for dtype in (torch.float32, torch.bfloat16):
                    x = x32.to(dev).to(dtype)
                    buf = torch.zeros(n + 1, device=dev, dtype=dtype)
                    buf[1:] = x
                    xm = buf[1:]  # contiguous, off every 16-byte boundary
                    tag = f"{shape} {str(dtype)[6:]} {logits} {labels}"
                    nbuf = same(f"{tag} lss_bce_logits+bwd", lambda lib: train(lib, "bce", x, t, plane, K, pw))
                    nbuf += same(f"{tag} lss_bce_logits_pc+bwd", lambda lib: train(lib, "pc", x, t, plane, K, pwc))
                    nbuf += same(f"{tag} lss_focal_logits_pc+bwd", lambda lib: train(lib, "focal", x, t, plane, K, rows))
                    ncall = 3
                    for mname, valid in masks.items():
                        nbuf += same(f"{tag} lss_seg_loss_masked+bwd {mname}",
                                     lambda lib: train(lib, "masked", x, t, plane, K, rows, valid))
                        ncall += 1
                    for nv in (0, (B + 1) // 2, B, "misaligned"):
                        xs = xm if nv == "misaligned" else x
                        n_valid = None if nv == "misaligned" else torch.tensor([nv], device=dev, dtype=torch.int32)
                        nbuf += same(f"{tag} lss_bce_iou_accum n_valid {nv}",
                                     lambda lib: accum(lib, "iou", xs, t, B, plane, K, pw, n_valid))
                        nbuf += same(f"{tag} lss_bce_iou_accum_pc n_valid {nv}",
                                     lambda lib: accum(lib, "iou_pc", xs, t, B, plane, K, pwc, n_valid))
                        nbuf += same(f"{tag} lss_seg_metrics_accum n_valid {nv}",
                                     lambda lib: accum(lib, "seg", xs, t, B, plane, K, rows, n_valid, thetas))
                        ncall += 3
                        for mname, valid in masks.items():
                            nbuf += same(f"{tag} lss_seg_metrics_accum_masked n_valid {nv} {mname}",
                                         lambda lib: accum(lib, "seg_masked", xs, t, B, plane, K, rows, n_valid, thetas, valid))
                            ncall += 1
                    print(f"{tag}: {ncall} calls, {nbuf} buffers equal", flush=True)
                    cases, calls = cases + 1, calls + ncall
    print(f"loss_ab: {cases} cases, {calls} calls, every output buffer equal byte for byte", flush=True)
    if a.skip_times:
        return 0

    # ---- part 2
    B, K, plane = 8, 8, 200 * 200
    n = B * K * plane
    torch.manual_seed(0)
    x = torch.randn(n, device=dev).bfloat16()
    t = (torch.rand(n, device=dev) < 0.03).float()
    valid = (torch.rand(B, plane, device=dev) < 0.7).to(torch.uint8)
    pwc = torch.tensor([1.0 + 0.5 * k for k in range(K)], **f32)
    rows = torch.stack([pwc, torch.ones_like(pwc), torch.full_like(pwc, 2.0)], dim=1).contiguous()
    n_valid = torch.tensor([B], device=dev, dtype=torch.int32)
    tb, ab = (lambda kind: lambda lib: train_bufs(lib, kind, x)), (lambda kind: lambda lib: accum_bufs(lib, kind, n, K))
    items = {  # name: (the output buffers, allocated once and shared by the two libraries; the calls)
        "lss_bce_logits + bwd": (tb("bce"), lambda lib, o: train(lib, "bce", x, t, plane, K, 2.13, o=o)),
        "lss_bce_logits_pc + bwd": (tb("pc"), lambda lib, o: train(lib, "pc", x, t, plane, K, pwc, o=o)),
        "lss_focal_logits_pc + bwd": (tb("focal"), lambda lib, o: train(lib, "focal", x, t, plane, K, rows, o=o)),
        "lss_seg_loss_masked + bwd": (tb("masked"), lambda lib, o: train(lib, "masked", x, t, plane, K, rows, valid, o=o)),
        "lss_bce_iou_accum": (ab("iou"), lambda lib, o: accum(lib, "iou", x, t, B, plane, K, 2.13, n_valid, o=o)),
        "lss_bce_iou_accum_pc": (ab("iou_pc"), lambda lib, o: accum(lib, "iou_pc", x, t, B, plane, K, pwc, n_valid, o=o)),
        "lss_seg_metrics_accum": (ab("seg"), lambda lib, o: accum(lib, "seg", x, t, B, plane, K, rows, n_valid, thetas, o=o)),
        "lss_seg_metrics_accum_masked": (ab("seg_masked"), lambda lib, o: accum(lib, "seg_masked", x, t, B, plane, K, rows,
                                                                               n_valid, thetas, valid, o=o))}
    print(f"\n{'entry, (8, 8, 200, 200) bf16':32s} {'parent median':>14s} {'min':>8s} {'max':>8s} {'this median':>12s} "
          f"{'min':>8s} {'max':>8s}   (us per graph replay; {a.rounds} x {a.replays} replays, alternating)")
    slower = []
    for name, (bufs, fn) in items.items():
        graphs = {}
        o = bufs(libs["this"])
        for side, lib in libs.items():
            sd = torch.cuda.Stream()
            sd.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(sd):
                for _ in range(3):
                    fn(lib, o)
            torch.cuda.current_stream().wait_stream(sd)
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                fn(lib, o)
            graphs[side] = (gr, o)
        times = {side: [] for side in graphs}
        for r in range(a.rounds):
            for side, (gr, _) in (list(graphs.items())[::-1] if r % 2 else graphs.items()):
                gr.replay()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(a.replays):
                    gr.replay()
                t1.record()
                torch.cuda.synchronize()
                times[side].append(t0.elapsed_time(t1) * 1e3 / a.replays)
        med = {side: statistics.median(v) for side, v in times.items()}
        good = med["this"] <= max(times["parent"])
        if not good:
            slower.append(name)
        print(f"{name:32s} {med['parent']:14.2f} {min(times['parent']):8.2f} {max(times['parent']):8.2f} "
              f"{med['this']:12.2f} {min(times['this']):8.2f} {max(times['this']):8.2f}   {'ok' if good else 'SLOWER'}",
              flush=True)
    if slower:
        print("loss_ab: this tree's median is above the parent's slowest round for: " + ", ".join(slower))
        return 3
    print("loss_ab: every entry's median is no higher than the parent's slowest round")
    return 0


if __name__ == "__main__":
    sys.exit(main())
