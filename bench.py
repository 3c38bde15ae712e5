"""LSS fwd+bwd frames/sec (BASELINE.json metric) on 1..8 MI355X, one process per GPU.

Workload (default: config 3 of BASELINE.json): B=8 samples x 6 cameras x 128x352 per GPU, D=41,
200x200 BEV, bf16 autocast, the full training step of train_simbev.py:229-248 (forward, SimpleLoss,
backward, clip_grad_norm_(5.0), Adam step). Synthetic SimBEV-shaped inputs,
random-init weights. The step is replayed as two HIP graphs (train_step.TrainStep: fwd+loss+bwd |
clip+Adam) with one RCCL all-reduce of the flat fp32 gradient between them; the camera inverses are
the host's torch.inverse (src/models.py:180,186), staged into the graph's static inputs before each
replay (ops.HostInverses). --graph 0 runs the step eagerly (DDP for N>1).

  python bench.py                          # N=1, config 3
  python bench.py --gpus 8                 # launches 8 ranks (torchrun) itself, B=8 per rank
  python bench.py --config c2              # config 2: B=4, fp32, forward only
  python bench.py --config c5              # config 5 per-GPU shard: B=4, 256x704, D=60, 400x400
  python bench.py --dump-outputs DIR       # also one more step from the initial state, its outputs as DIR/<name>.npy
  python bench.py --full                   # also the roofline and the CPU baseline (below)

A plain run sets up, warms up, times `--steps` steps and prints the result line (metric, value, unit,
ms_per_step, the configuration). Everything below takes runs of its own and is measured with --full only.

With --full, also reported on the same JSON line:
  roofline      the splat forward kernel (lss_splat_fwd): algorithmic bytes per launch / its average
                launch time (kernel-stamped hipEvents on its own stream) vs 8 TB/s HBM peak; `traffic`
                = HBM bytes per launch from rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes over the
                same kernel and shapes, run by this script (scripts/splat_pmc.py, before the GPU is
                touched here), FETCH_SIZE doubled per the gfx950 correction of MI355X_MICROARCH.md
  cpu_baseline  the CPU oracle (restatement of the reference's path, fp32 eager, same conv stacks)
                timed on this host, rank 0, N=1 only: full-model training steps and the hot path
                alone, at the config 3 shape and at config 1; `value` = full model at config 3
"""
from __future__ import annotations

import argparse
import csv
import glob
import hashlib
import json
import os
import shutil
import socket
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)


def miopen_dirs(repo: str) -> tuple:
    """(user db, kernel cache) for MIOpen. MIOpen rewrites its user databases while it runs, so it
    gets a working copy of the committed ones (tuning/miopen/db) under the git-ignored cache
    directory, refreshed when a committed file is newer; the committed files stay as checked out.
    Where the tree cannot be written (a read-only checkout), both live in a per-user directory under
    the system's temporary directory instead."""
    src = os.path.join(repo, "tuning", "miopen", "db")
    in_tree = os.path.join(repo, "tuning", "miopen", "cache")
    tag = hashlib.sha1(os.path.abspath(repo).encode()).hexdigest()[:10]  # one directory per checkout and user
    for cache in (in_tree, os.path.join(tempfile.gettempdir(), f"lss_miopen_{os.getuid()}_{tag}")):
        db = os.path.join(cache, "db")
        try:
            os.makedirs(db, mode=0o700, exist_ok=True)
            if not os.access(db, os.W_OK):
                raise PermissionError(db)
            for name in os.listdir(src):
                s, d = os.path.join(src, name), os.path.join(db, name)
                if not os.path.exists(d) or os.path.getmtime(s) > os.path.getmtime(d):
                    tmp = f"{d}.{os.getpid()}.tmp"  # (several ranks may start at once: the copy appears whole)
                    shutil.copyfile(s, tmp)
                    os.replace(tmp, d)
            return db, cache
        except OSError:
            continue
    return src, in_tree  # nowhere to write: MIOpen reads the committed databases and keeps nothing


# MIOpen find results (which conv solver per shape) and compiled kernels, kept in-tree so a
# fresh box does not repeat the exhaustive search (tuning/README.md). Must precede torch init.
if "MIOPEN_USER_DB_PATH" not in os.environ or "MIOPEN_CUSTOM_CACHE_DIR" not in os.environ:
    _db, _cache = miopen_dirs(REPO)
    os.environ.setdefault("MIOPEN_USER_DB_PATH", _db)
    os.environ.setdefault("MIOPEN_CUSTOM_CACHE_DIR", _cache)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

FORCE_PG = os.environ.get("LSS_BENCH_FORCE_PG", "0") == "1"  # rehearse the N>1 collectives on one GPU
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec (MI355X_MICROARCH.md, chip-level parameters)
METRIC = "LSS fwd+bwd frames/sec at B=8, 6×128×352, D=41 → 200×200 BEV; 1/2/4/8 GPU"


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", default="c3", choices=["c1", "c2", "c3", "c4", "c5"])
    ap.add_argument("--batch", type=int, default=0, help="samples per GPU (0: the config's)")
    ap.add_argument("--mode", default="auto", choices=["auto", "train", "fwd"],
                    help="auto: forward only for config 2 (fp32), the full training step otherwise")
    ap.add_argument("--dtype", default="", choices=["", "bf16", "fp32"])
    ap.add_argument("--bev-layout", default="", choices=["", "nhwc", "nchw"])
    ap.add_argument("--trunk-channels-last", type=int, default=0)
    ap.add_argument("--up1-channels-last", type=int, default=1)
    ap.add_argument("--dw-impl", default="hip", choices=["hip", "miopen", "native", "fp32"],
                    help="depthwise convs of the trunk: HIP kernels, MIOpen, PyTorch native, MIOpen in fp32")
    ap.add_argument("--miopen-find", type=int, default=-1,
                    help="torch.backends.cudnn.benchmark: 1 = MIOpen's find times every applicable solver per conv "
                         "shape in this process (~30 s in the first step), 0 = MIOpen picks from the find results "
                         "recorded in tuning/miopen/db (same kernels, no search); default: 1 with --full, else 0")
    ap.add_argument("--hip-bn", type=int, default=1, help="BatchNorm + activation on the lss_bn_* kernels")
    ap.add_argument("--fuse-depthnet", type=int, default=1, help="depthnet 1x1 conv inside the lift kernel (MFMA)")
    ap.add_argument("--bn-relu-y", default="recompute", choices=("recompute", "keep"),
                    help="channels-last BN + ReLU without a residual: the backward recomputes the output from x "
                         "or keeps and re-reads it")
    ap.add_argument("--hip-adam", type=int, default=1,
                    help="clip_grad_norm_ + Adam as two lss_clip_adam launches (0: torch's foreach norm and fused Adam)")
    ap.add_argument("--hip-pw", type=int, default=2,
                    help="trunk 1x1 convs: 2 = forward/backward-data on lss_pw_conv and weight gradients on lss_pw_wrw, "
                         "1 = lss_pw_wrw only, 0 = MIOpen")
    ap.add_argument("--flip-bwd", type=int, default=1,
                    help="stride-1 3x3 convs: backward-data as a forward conv of the flipped weight (models.USE_FLIP_BWD)")
    ap.add_argument("--plan-at", default="dropout", choices=("trunk", "dropout", "lift"),
                    help="plan kernels in front of the trunk, the dropout or the fused lift")
    ap.add_argument("--plan-ordered", type=int, default=1,
                    help="ordered plans (geometry + scan + scatter to canonical positions); 0: the four-kernel plan "
                         "with k_csr_canon")
    ap.add_argument("--hip-dropout", type=int, default=1,
                    help="CamEncode.dropout on lss_dropout (written where the fused lift reads it) instead of torch's")
    ap.add_argument("--graph", type=int, default=1,
                    help="replay the step as HIP graphs (fwd+bwd, clip+Adam) with the gradient all-reduce "
                         "between them; 0 = eager (DDP for N>1)")
    ap.add_argument("--overlap-all-reduce", type=int, default=1,
                    help="N>1: one flat master per backward group (BevEncode, trunk head, trunk), each all-reduced "
                         "from its gradient hook on a side stream inside the captured backward")
    ap.add_argument("--param-groups", type=int, default=1,
                    help="with --flat-params: one flat master per backward group (BevEncode, trunk head, trunk) "
                         "at any world size, each group's gradient gathered as soon as the backward completes it")
    ap.add_argument("--flat-params", type=int, default=1,
                    help="trainable parameters as one fp32 master tensor with one bf16 working copy per step")
    ap.add_argument("--full", action="store_true",
                    help="after the headline figure also measure the roofline of the splat kernels (--profile-steps, "
                         "--in-graph-prof, --pmc-traffic, the write ceiling) and the CPU baseline (--cpu-baseline)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="after the timed steps the timed step is called once more from the run's initial parameters, "
                         "optimizer state and seed (training is chaotic: only then are its outputs the same from run "
                         "to run), and rank 0 writes what that call computed as DIR/<name>.npy (float32): the value "
                         "it returns (loss, or preds of a forward-only step) and, for a training step, the gradients "
                         "(flattened; a fixed seeded sample when large)")
    ap.add_argument("--profile-steps", type=int, default=20,
                    help="--full: steps after the timed region over which the splat kernel's time is averaged")
    ap.add_argument("--in-graph-prof", type=int, default=1,
                    help="--full, rank 0, N=1, hipgraph: also time the splat inside the captured step's replays with a "
                         "rocprofv3 --kernel-trace child run of this script (before this process touches the GPU)")
    ap.add_argument("--watchdog", type=float, default=0.0,
                    help="seconds after which a rank that has not finished exits non-zero (0: 300 + 2 s per step)")
    ap.add_argument("--pmc-traffic", type=int, default=1,
                    help="--full: rocprofv3 FETCH_SIZE/WRITE_SIZE passes (rank 0, N=1)")
    ap.add_argument("--cpu-baseline", type=int, default=1, help="--full: time the CPU oracle (rank 0, N=1, config 3)")
    ap.add_argument("--cpu-runs", type=int, default=3, help="timed CPU runs per case (median; 1 warm-up before)")
    ap.add_argument("--caller", default="bench", choices=("bench", "reference"),
                    help="reference: the unchanged train_simbev.py loop (train_simbev.py:229-248) -- compile_model "
                         "with the package defaults, fp32, eager, torch Adam + clip_grad_norm_, the host inverse "
                         "per forward; overrides --dtype/--graph/--flat-params/--hip-adam and the kernel switches")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if not args.full:  # a plain run measures the headline figure only
        args.profile_steps = args.in_graph_prof = args.pmc_traffic = args.cpu_baseline = 0
    if args.miopen_find < 0:
        args.miopen_find = int(args.full)
    if args.caller == "reference":
        args.mode, args.dtype, args.graph, args.flat_params, args.hip_adam = "train", "fp32", 0, 0, 0
    cfg_b = {"c1": 1, "c2": 4, "c3": 8, "c4": 8, "c5": 4}[args.config]
    args.batch = args.batch or cfg_b
    if args.mode == "auto":
        args.mode = "fwd" if args.config == "c2" else "train"
    if not args.dtype:
        args.dtype = "fp32" if args.mode == "fwd" else "bf16"
    if not args.bev_layout:
        args.bev_layout = "nhwc"  # the module default (models.LiftSplatShoot.bev_layout)
    return args


def free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def maybe_launch_ranks(args) -> None:
    """`--gpus N` without a torchrun environment: launch N ranks (one process per GPU) through
    torch.distributed.run as a child process -- before this process touches the GPU -- and exit with
    its status. Rank 0 of the child job prints the JSON line."""
    if args.gpus <= 1 or "WORLD_SIZE" in os.environ:
        return
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    log(f"[bench] launching {args.gpus} ranks: {' '.join(cmd)}")
    sys.exit(subprocess.call(cmd, env=env))


def setup_dist(args):
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        log(f"[rank {rank}] note: --gpus {args.gpus} but WORLD_SIZE={world}; reporting the job's {world} ranks")
    if world > 1:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        torch.cuda.set_device(local)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    elif FORCE_PG:
        # one-GPU rehearsal of the N>1 step: a world-size-1 RCCL group, collectives issued anyway
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(free_port()))
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    else:
        torch.cuda.set_device(0)
    return world, rank, torch.device("cuda", local if world > 1 else 0)


def splat_fwd_bytes(B, N, D, H, W, X, Y, Z, kept, out_bytes, ctx_bytes) -> int:
    """Algorithmic bytes of one lss_splat_fwd launch (Roofline)."""
    nprime = B * N * D * H * W
    ncells = B * Z * X * Y
    return (nprime * 4                    # depth weights (fp32), one per point
            + B * N * H * W * 64 * ctx_bytes  # context rows (the depthnet output's type: bf16 under autocast)
            + kept * 4                    # sorted point ids
            + (ncells + 1) * 4            # cell_start
            + ncells * 64 * out_bytes)    # dense BEV, every element written once


def splat_fwd_bytes_survey(B, N, D, H, W, X, Y, Z, in_bytes, out_bytes) -> int:
    """SURVEY.md §8(d)'s fused-forward formula: the depthnet output (D + C per pixel), one int32 voxel
    id per point, the dense BEV (for comparison with splat_fwd_bytes, which counts what this
    kernel reads: depth weights, context rows, sorted point ids and cell starts)."""
    return B * N * H * W * (D + 64) * in_bytes + B * N * D * H * W * 4 + B * 64 * Z * X * Y * out_bytes


def splat_bwd_bytes(B, N, D, H, W, occupied, in_bytes, g_bytes) -> dict:
    """Algorithmic HBM bytes of one lss_splat_bwd launch (k_splat_bwd_tile): per pixel its
    D depth weights (fp32) and cell ids (int32), its context row (C values) and its d_depthnet_out
    row (D + C values); per occupied BEV cell its gradient row (C values, read once from HBM; every
    further kept point of the cell re-reads it from L2 / MALL: `gather_bytes`)."""
    pix = B * N * H * W
    hbm = pix * (D * 4 * 2 + 64 * in_bytes + (D + 64) * in_bytes) + occupied * 64 * g_bytes
    return {"hbm": hbm, "per_pixel": D * 8 + 64 * in_bytes + (D + 64) * in_bytes, "occupied_rows": occupied,
            "row_bytes": 64 * g_bytes}


def write_ceiling(numel, dtype, dev, reps=10) -> dict:
    """Measured HBM write ceiling for the splat's output buffer: lss_ceiling_store, a hand-written
    16-B streaming-store kernel (consecutive lanes on consecutive 16 B, `per_thread` stores per lane,
    non-temporal or plain) over a BEV-sized buffer, kernel-stamped events (the kernel alone), mean
    over `reps` launches, each after a 512 MiB read sweep (lss_ceiling_read: L2 and the Infinity
    Cache hold clean lines, as after the trunk's reads; the ceiling) and after a 512 MiB write (dirty
    lines the stores must evict first; reported beside it). The fastest store form is the ceiling.
    Also the torch memset (fill kernel) and copy (read + write) of the same buffer, read-swept."""
    import ctypes as ct
    from lss_carla_amd import _lib
    lib = _lib.load()
    buf = torch.empty(numel, dtype=dtype, device=dev)
    src = torch.empty_like(buf)
    nbytes = numel * buf.element_size()
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    sink = torch.zeros(4, dtype=torch.int32, device=dev)
    st = _lib.stream_handle(dev)

    def prepare(state):
        if state == "read":
            _lib.check(lib.lss_ceiling_read(_lib.ptr(flush), flush.numel(), _lib.ptr(sink), st), "ceiling_read")
        else:
            flush.zero_()

    def stamped(per_thread, flavor, state) -> float:
        tot = 0.0
        for i in range(reps + 2):
            prepare(state)
            a, b = ct.c_void_p(), ct.c_void_p()
            lib.lss_event_create(ct.byref(a))
            lib.lss_event_create(ct.byref(b))
            _lib.check(lib.lss_ceiling_store(_lib.ptr(buf), nbytes, per_thread, flavor, st, a, b), "ceiling_store")
            ms = ct.c_float()
            lib.lss_event_elapsed_ms(a, b, ct.byref(ms))
            lib.lss_event_destroy(a)
            lib.lss_event_destroy(b)
            if i >= 2:
                tot += ms.value
        return tot / reps * 1e3

    def timed(fn) -> float:
        tot = 0.0
        for i in range(reps + 2):
            prepare("read")
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= 2:
                tot += e0.elapsed_time(e1)
        return tot / reps * 1e3

    forms = {}
    for pt in CEILING_PER_THREAD:
        for fl, fname in ((1, "nt"), (0, "plain"), (2, "sc1")):
            forms[f"pt{pt}_{fname}"] = {"read": round(stamped(pt, fl, "read"), 2),
                                        "dirty": round(stamped(pt, fl, "dirty"), 2)}
    best = min(forms, key=lambda k: forms[k]["read"])
    us = forms[best]["read"]
    us_memset = timed(lambda: buf.zero_())
    us_copy = timed(lambda: buf.copy_(src))  # the copy-kernel ceiling SURVEY 8(d) asks for: read + write
    del buf, src, flush
    return {"what": f"lss_ceiling_store: 16-B streaming stores over the {nbytes / 1e6:.1f} MB BEV buffer after a "
                    f"512 MiB read sweep, fastest form ({best}); kernel-stamped events",
            "us": round(us, 2), "GB/s": round(nbytes / us / 1e3, 1), "form": best, "forms_us": forms,
            "dirty_us": forms[best]["dirty"], "dirty_GB/s": round(nbytes / forms[best]["dirty"] / 1e3, 1),
            "memset_us": round(us_memset, 2), "memset_GB/s": round(nbytes / us_memset / 1e3, 1),
            "copy_us": round(us_copy, 2), "copy_GB/s": round(2 * nbytes / us_copy / 1e3, 1)}


CEILING_PER_THREAD = (1, 4)


# ----------------------------------------------------------------------------- HBM traffic (PMC)
def measure_traffic(args, B) -> dict | None:
    """FETCH_SIZE and WRITE_SIZE of lss_splat_fwd per launch (rocprofv3, one pass per counter group),
    on scripts/splat_pmc.py with this run's config / batch / dtype / layout. Runs child processes
    before this process initialises the GPU; returns None if rocprofv3 is unavailable or fails."""
    prof = shutil.which("rocprofv3")
    if prof is None:
        return None
    out = {}
    tmp = tempfile.mkdtemp(prefix="lss_pmc_", dir="/tmp")
    env = dict(os.environ, TMPDIR="/tmp")
    for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
        d = os.path.join(tmp, ctr)
        cmd = ["timeout", "-s", "KILL", "150", prof, "--pmc", ctr, "--kernel-include-regex", "k_splat_fwd",
               "--output-format", "csv", "-d", d, "-o", "run", "--", sys.executable,
               os.path.join(REPO, "scripts", "splat_pmc.py"), "--config", args.config, "--batch", str(B),
               "--dtype", args.dtype, "--layout", args.bev_layout]
        try:
            r = subprocess.run(cmd, cwd="/tmp", env=env, capture_output=True, text=True, timeout=170)
        except subprocess.TimeoutExpired:
            log(f"[bench] rocprofv3 {ctr} pass timed out")
            return None
        files = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)
        if r.returncode != 0 or not files:
            log(f"[bench] rocprofv3 {ctr} pass failed (rc={r.returncode}): {r.stderr[-400:]}")
            return None
        vals = []
        for f in files:
            with open(f) as fh:
                for row in csv.DictReader(fh):
                    if "k_splat_fwd" in row["Kernel_Name"] and row["Counter_Name"] == ctr:
                        vals.append(float(row["Counter_Value"]))
        if not vals:
            return None
        vals = vals[2:] if len(vals) > 4 else vals  # first launches: cold caches, one-time page mapping
        out[ctr] = sum(vals) / len(vals) * 1024.0  # counters are in KiB
    shutil.rmtree(tmp, ignore_errors=True)
    return {"fetch_bytes_raw": round(out["FETCH_SIZE"]), "write_bytes": round(out["WRITE_SIZE"]),
            "hbm_bytes_per_launch": round(2 * out["FETCH_SIZE"] + out["WRITE_SIZE"])}


def measure_in_graph(args) -> dict | None:
    """The splat's kernel time inside the captured step: a rocprofv3 --kernel-trace child run of this
    script (same config, 10 timed replays, no eager profile steps), the k_splat_fwd launches of those
    replays. Runs before this process initialises the GPU; None if rocprofv3 is missing or fails."""
    prof = shutil.which("rocprofv3")
    if prof is None or not args.graph:
        return None
    tmp = tempfile.mkdtemp(prefix="lss_trace_", dir="/tmp")
    steps = 30  # (10 replays left the average ±1 us from run to run on one box)
    cmd = ["timeout", "-s", "KILL", "280", prof, "--kernel-trace", "--output-format", "csv", "-d", tmp, "-o", "run",
           "--", sys.executable, os.path.abspath(__file__), "--config", args.config, "--batch", str(args.batch),
           "--dtype", args.dtype, "--bev-layout", args.bev_layout, "--steps", str(steps), "--warmup", "3",
           "--full", "--profile-steps", "0", "--pmc-traffic", "0", "--cpu-baseline", "0", "--in-graph-prof", "0",
           "--mode", args.mode]
    # the rest of this run's configuration, so the child measures the same step
    for flag in ("miopen_find", "hip_bn", "bn_relu_y", "hip_adam", "fuse_depthnet", "hip_dropout", "hip_pw", "plan_at",
                 "flip_bwd",
                 "plan_ordered", "trunk_channels_last", "up1_channels_last", "param_groups",
                 "flat_params", "overlap_all_reduce", "dw_impl"):
        cmd += ["--" + flag.replace("_", "-"), str(getattr(args, flag))]
    try:
        # the child's progress lines pass through to this process's stderr (no long silence)
        r = subprocess.run(cmd, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), stdout=subprocess.DEVNULL,
                           stderr=None, text=True, timeout=300)
    except subprocess.TimeoutExpired:
        log("[bench] in-graph kernel trace timed out")
        return None
    files = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
    if r.returncode != 0 or not files:
        log(f"[bench] in-graph kernel trace failed (rc={r.returncode})")
        return None
    rows = {"splat": [], "lift": [], "bwd": []}
    for f in files:
        with open(f) as fh:
            for row in csv.DictReader(fh):
                k = row["Kernel_Name"]
                key = ("splat" if "k_splat_fwd" in k else "bwd" if "k_splat_bwd" in k
                       else "lift" if ("k_depthnet_lift" in k or "k_lift_prep" in k) else None)
                if key:
                    rows[key].append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
    shutil.rmtree(tmp, ignore_errors=True)
    for v in rows.values():
        v.sort()
    # the last launch is the eager step after the replays; the `steps` before it are the timed replays
    sel = rows["splat"][-1 - steps:-1]
    if len(sel) < steps:
        return None
    durs = [(e - b) / 1e3 for b, e in sel]
    res = {"us": round(sum(durs) / len(durs), 2), "min_us": round(min(durs), 2), "launches": len(durs),
           "how": f"rocprofv3 --kernel-trace of a child run of this script: the {steps} timed graph replays"}
    # what the splat adds to the step after the lift: the lift kernel's end to the splat's end (the
    # kernel plus the launch gap in front of it)
    # (the lift launched last before the splat; trace timestamps of back-to-back kernels can overlap
    # by a few ns, so the lift is found by its start)
    after = [(e - max((lb, le) for lb, le in rows["lift"] if lb <= b)[1]) / 1e3 for b, e in sel
             if any(lb <= b for lb, le in rows["lift"])]
    if after:
        res["after_lift_us"] = round(sum(after) / len(after), 2)
    # the splat backward of the same replays (training mode: one per step)
    bsel = rows["bwd"][-1 - steps:-1]
    if len(bsel) == steps:
        bd = [(e - b) / 1e3 for b, e in bsel]
        res["bwd"] = {"kernel": "k_splat_bwd", "us": round(sum(bd) / len(bd), 2), "min_us": round(min(bd), 2),
                      "launches": len(bd)}
    return res


# ----------------------------------------------------------------------------- CPU baseline
def cpu_threads() -> tuple:
    """Threads for the CPU baseline: the CPUs this process may run on, capped by the cgroup quota."""
    try:
        aff = len(os.sched_getaffinity(0))
    except AttributeError:
        aff = os.cpu_count() or 1
    quota = None
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, p = f.read().split()[:2]
            if q != "max":
                quota = max(1, int(int(q) // int(p)))
    except (OSError, ValueError):
        pass
    n = min(aff, quota) if quota else aff
    return n, {"os_cpu_count": os.cpu_count(), "affinity": aff, "cgroup_quota_cpus": quota}


def cpu_baseline(model, args) -> dict:
    """The reference path on the host (fp32 eager): the oracle's geometry/lift/splat (a restatement of
    src/models.py:170-246, src/tools.py:182-219) plus the same conv stacks. Full-model training steps
    (fwd + SimpleLoss + bwd + clip + Adam) and the hot path alone (depthnet output -> geometry, lift,
    splat -> sum().backward()), at the config 3 shape (B=8 x 6 cams) and at config 1; 1 warm-up, then
    the median of `cpu_runs` runs."""
    import copy
    import statistics

    from oracle import lss_ref as ref
    from lss_carla_amd import synthetic as syn
    import lss_carla_amd as L

    threads, tinfo = cpu_threads()
    torch.set_num_threads(threads)
    cpu_model = copy.deepcopy(model).to("cpu").float()
    cpu_model.static_inverses = None
    cpu_model.bevencode.to(memory_format=torch.contiguous_format)
    cpu_model.camencode.to(memory_format=torch.contiguous_format)
    cpu_model.train()
    loss_fn = L.SimpleLoss(2.13)
    opt = torch.optim.Adam(cpu_model.parameters(), lr=1e-3, weight_decay=1e-7)
    frustum = cpu_model.frustum.detach()

    def median_time(fn):
        fn()  # warm-up
        ts = []
        for _ in range(args.cpu_runs):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts)

    res = {}
    for name in ("c3", "c1"):
        cfg, gc, _ = syn.config_confs(name)
        B, N, fd = cfg["B"], cfg["N"], cfg["final_dim"]
        dx, bx, nx = ref.gen_dx_bx(gc["xbound"], gc["ybound"], gc["zbound"])
        rig = syn.make_rig(B, N, fd, seed=0)
        imgs = syn.make_images(B, N, fd)
        labels = syn.make_labels(B, int(nx[0]), int(nx[1]))
        fr = ref.create_frustum(fd, gc["dbound"]) if name != args.config else frustum
        D, H, W = fr.shape[:3]
        dn = syn.make_depthnet_out(B, N, D, H, W, seed=0).requires_grad_(True)

        def full_step():
            opt.zero_grad()
            out = ref.full_forward(cpu_model.camencode.depthnet_out, cpu_model.bevencode, fr, imgs, rig["rots"],
                                   rig["trans"], rig["intrins"], rig["post_rots"], rig["post_trans"], dx, bx, nx, D)
            loss_fn(out, labels).backward()
            torch.nn.utils.clip_grad_norm_(cpu_model.parameters(), 5.0)
            opt.step()

        def hot_path():
            dn.grad = None
            ref.get_voxels(fr, dn, rig["rots"], rig["trans"], rig["intrins"], rig["post_rots"], rig["post_trans"],
                           dx, bx, nx, D).sum().backward()

        t_hot = median_time(hot_path)
        t_full = median_time(full_step)
        res[name] = {"B": B, "N": N, "full_model_frames_per_s": round(B / t_full, 4),
                     "hot_path_frames_per_s": round(B / t_hot, 3),
                     "full_step_s": round(t_full, 4), "hot_path_s": round(t_hot, 5)}
    return {"value": res["c3"]["full_model_frames_per_s"], "unit": "frames/s", "cores": threads, "kind": "port",
            "sample": (f"full training steps (fwd+loss+bwd+clip+Adam) at the config 3 shape, B=8 x 6 cams x "
                       f"128x352, fp32 eager, oracle lift/splat + the same conv stacks; {threads} threads "
                       f"({tinfo}); 1 warm-up + median of {args.cpu_runs}"),
            "detail": res}


# ----------------------------------------------------------------------------- model / steps
def build_model(args, dev, gc, dac):
    import lss_carla_amd as L

    model = L.compile_model(gc, dac, outC=1).to(dev)
    model.bev_layout = args.bev_layout
    model.fuse_depthnet = bool(args.fuse_depthnet)
    if args.bev_layout == "nhwc":
        model.bevencode.to(memory_format=torch.channels_last)
    if args.trunk_channels_last:
        model.camencode.to(memory_format=torch.channels_last)
    elif args.up1_channels_last:
        # CamEncode.up1's 3x3 convs see channels-last maps: channels-last weights spare MIOpen's weight
        # copy per forward and the layout-changing gradient copy into the flat parameters
        model.camencode.up1.to(memory_format=torch.channels_last)
    from lss_carla_amd import norm, models
    norm.USE_HIP_BN = bool(args.hip_bn)
    norm.RECOMPUTE_RELU_Y = args.bn_relu_y == "recompute"
    from lss_carla_amd import optim as lss_optim
    lss_optim.USE_HIP_ADAM = bool(args.hip_adam)
    models.USE_HIP_DROPOUT = bool(args.hip_dropout)
    models.PLAN_AT = args.plan_at
    models.USE_FLIP_BWD = bool(args.flip_bwd)
    from lss_carla_amd import efficientnet
    efficientnet.USE_HIP_PW_WRW = args.hip_pw >= 1
    efficientnet.USE_HIP_PW_GEMM = args.hip_pw >= 2
    from lss_carla_amd.efficientnet import set_depthwise_impl
    set_depthwise_impl(model.camencode.trunk, args.dw_impl)
    model.train() if args.mode == "train" else model.eval()
    return model


class ReferenceCallerStep:
    """One iteration of the reference's training loop as written (train_simbev.py:229-248): zero_grad,
    forward with `.to(device)` on every input (no-ops: the batch is resident before the timed region),
    SimpleLoss, backward, clip_grad_norm_(5.0), torch Adam (its default implementation) step."""

    def __init__(self, model, inputs, labels, loss_fn, opt, dev):
        self.model, self.inputs, self.labels, self.loss_fn, self.opt, self.dev = model, inputs, labels, loss_fn, opt, dev

    def __call__(self):
        self.opt.zero_grad()
        preds = self.model(*[t.to(self.dev) for t in self.inputs])
        loss = self.loss_fn(preds, self.labels.to(self.dev))
        loss.backward()
        torch.nn.utils.clip_grad_norm_(self.model.parameters(), 5.0)
        self.opt.step()
        return preds

    eager = __call__


class FwdStep:
    """Forward only (config 2): the model's forward under no_grad, eager or replayed as one HIP graph."""

    def __init__(self, model, inputs, pre_step=None):
        self.model, self.inputs, self.pre_step = model, inputs, pre_step
        self.graph = None
        self.out = None

    def eager(self):
        if self.pre_step is not None:
            self.pre_step()
        with torch.no_grad():
            self.out = self.model(*self.inputs)
        return self.out

    def capture(self, warmup, on_warmup=None):
        dev = self.inputs[0].device
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for i in range(max(warmup, 1)):
                self.eager()
                if on_warmup is not None:
                    on_warmup(i)
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph), torch.no_grad():
            self.out = self.model(*self.inputs)

    def __call__(self):
        if self.graph is None:
            return self.eager()
        if self.pre_step is not None:
            self.pre_step()
        self.graph.replay()
        return self.out


DUMP_MAX_ELEMS = 6 << 20  # per array (24 MiB of float32): the dump stays under 64 MB


def step_params(step) -> list:
    """The tensors a training step's optimizer updates (TrainStep.params, or the reference caller's
    model.parameters()), in the optimizer's order; [] for a forward-only step."""
    if isinstance(step, FwdStep):
        return []
    return list(step.params) if hasattr(step, "params") else [p for p in step.model.parameters() if p.requires_grad]


def restore_initial(step, snap, seed: int) -> None:
    """Put a training step back where the run began: the parameters' initial values (`snap`, cloned
    before the first step) copied in place, the Adam state zeroed in place (a fresh Adam's state: the
    captured graphs keep reading the same tensors) and torch's generators reseeded (the dropout and
    drop-connect draws). Training is chaotic: MIOpen's and the kernels' atomic reductions differ in
    the last bits from run to run, and after a few Adam steps (a sign-like update where a gradient is
    near zero) two runs' parameters are 1e-2 apart. One step from this state is reproducible."""
    with torch.no_grad():
        for p, s in zip(step_params(step), snap):
            p.copy_(s)
        for st in step.opt.state.values():
            for k, v in st.items():
                if isinstance(v, torch.Tensor):
                    v.zero_()
                elif isinstance(v, (int, float)):
                    st[k] = type(v)(0)
    torch.manual_seed(seed)


def collect_outputs(step, out, mode) -> dict:
    """What a call of the timed step computed, as host float32 arrays: the value it returned (the
    loss of a training step, the preds of a forward-only or reference-caller step) and, for a
    training step, the gradients it updated the parameters with, flattened in the optimizer's order.
    (Not the updated parameters: Adam's first update is lr * g / (|g| + eps), a sign where g is near
    zero, so they are no continuous function of the step's inputs.) An array of more than
    DUMP_MAX_ELEMS elements is stored as a fixed sample (indices from a seeded generator, the same
    for every run and build)."""
    import numpy as np

    def host(ts):
        flat = torch.cat([t.detach().reshape(-1).float() for t in ts]).cpu().numpy()
        if flat.size > DUMP_MAX_ELEMS:
            idx = np.sort(np.random.default_rng(0).integers(0, flat.size, DUMP_MAX_ELEMS))
            flat = flat[idx]
        return np.ascontiguousarray(flat, dtype=np.float32)

    name = "preds" if isinstance(step, (FwdStep, ReferenceCallerStep)) else "loss"
    arrays = {name: out.detach().float().cpu().numpy().astype(np.float32)}
    if mode == "train":
        params = step_params(step)
        grads = getattr(step, "graph_grads", None) or [p.grad for p in params]
        arrays["grads"] = host([g if g is not None else torch.zeros_like(p) for g, p in zip(grads, params)])
    return arrays


def write_outputs(arrays: dict, d: str) -> None:
    import numpy as np
    os.makedirs(d, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(d, name + ".npy"), a)
    log(f"[rank 0] wrote {', '.join(f'{k}.npy {v.shape}' for k, v in arrays.items())} to {d}")


def start_watchdog(seconds: float, rank: int):
    """A rank that is still running after `seconds` (a hung collective or graph replay at N > 1) reports
    itself and exits non-zero -- no re-exec; the launcher then ends the job."""
    import threading

    def fire():
        log(f"[rank {rank}] watchdog: not finished after {seconds:.0f} s (hung replay or collective); exiting")
        os._exit(3)

    t = threading.Timer(seconds, fire)
    t.daemon = True
    t.start()
    return t


def main():
    args = parse()
    maybe_launch_ranks(args)
    # stdout carries exactly one line, the JSON result: anything else written to fd 1 from here on
    # (RCCL's version banner, library chatter) goes to stderr
    result_fd = os.dup(1)
    os.dup2(2, 1)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    from lss_carla_amd import synthetic as syn
    cfg, gc, dac = syn.config_confs(args.config)
    B, N, fd = args.batch, cfg["N"], cfg["final_dim"]
    traffic = None
    if args.pmc_traffic and world == 1 and rank == 0:
        t_p = time.perf_counter()
        traffic = measure_traffic(args, B)  # child processes, before this process touches the GPU
        log(f"[rank 0] splat PMC traffic {traffic} ({time.perf_counter() - t_p:.1f} s)")
    in_graph = None
    if args.in_graph_prof and args.graph and world == 1 and rank == 0:
        t_p = time.perf_counter()
        in_graph = measure_in_graph(args)  # a child process, before this process touches the GPU
        log(f"[rank 0] splat in the captured step: {in_graph} ({time.perf_counter() - t_p:.1f} s)")

    world, rank, dev = setup_dist(args)
    watchdog = start_watchdog(args.watchdog or 300.0 + 2.0 * (args.steps + args.warmup + args.profile_steps), rank)
    # (the unchanged caller leaves torch's default: no MIOpen find, train_simbev.py sets nothing)
    torch.backends.cudnn.benchmark = bool(args.miopen_find) and args.caller != "reference"
    from lss_carla_amd import ops, parallel
    if world > 1:
        parallel.control_group()  # the gloo group for collective decisions, created on every rank here
    from lss_carla_amd.flat_params import FlatParams, FlatParamGroups, lss_backward_groups
    from lss_carla_amd.train_step import TrainStep
    import lss_carla_amd as L

    torch.manual_seed(1234 + rank)
    ops.USE_PLAN_ORDERED = bool(args.plan_ordered)
    if args.caller == "reference":
        # train_simbev.py:184-185: compile_model(...).to(device), nothing else set
        model = L.compile_model(gc, dac, outC=1).to(dev)
        model.train()
    else:
        model = build_model(args, dev, gc, dac)
    amp_dtype = torch.bfloat16 if args.dtype == "bf16" else None
    rig_host = syn.make_rig(B, N, fd, seed=rank)
    rig = {k: v.to(dev) for k, v in rig_host.items()}
    imgs = syn.make_images(B, N, fd, seed=rank).to(dev)
    X, Y, Z = ops.GridSpec.from_conf(gc).nx
    labels = syn.make_labels(B, X, Y, seed=rank).to(dev)
    inputs = (imgs, rig["rots"], rig["trans"], rig["intrins"], rig["post_rots"], rig["post_trans"])

    pre_step = None
    if args.graph:
        # host torch.inverse of the (host) rig before every step, staged into the graph's static inputs
        hinv = ops.HostInverses(B * N, dev)
        model.static_inverses = (hinv.pinv, hinv.kinv)
        pinned = {k: rig_host[k].pin_memory() for k in ("post_rots", "intrins")}
        pre_step = lambda: hinv.update(pinned["post_rots"], pinned["intrins"])  # noqa: E731

    if args.caller == "reference":
        loss_fn = L.SimpleLoss(2.13).to(dev)
        opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-7)  # train_simbev.py:192
        step = ReferenceCallerStep(model, inputs, labels, loss_fn, opt, dev)
    elif args.mode == "train":
        flat = None
        if args.graph or args.flat_params:
            # one process per GPU without DDP: identical replicas, one flat gradient all-reduce
            parallel.broadcast_state(model)
            parallel.freeze_unused(model)
            overlap = bool(args.overlap_all_reduce) and (world > 1 or FORCE_PG)
            if args.flat_params and (overlap or args.param_groups):
                flat = FlatParamGroups(model, lss_backward_groups(), cast_dtype=amp_dtype)
            elif args.flat_params:
                flat = FlatParams(model, cast_dtype=amp_dtype)
        overlap = bool(args.overlap_all_reduce) and (world > 1 or FORCE_PG) and flat is not None
        if flat is not None:
            fwd, params = flat.bind(model), (flat.masters if isinstance(flat, FlatParamGroups) else [flat.master])
        else:
            fwd = model if (args.graph or world == 1) else parallel.make_data_parallel(model, dev)
            params = [p for p in model.parameters() if p.requires_grad]
        loss_fn = L.SimpleLoss(2.13).to(dev)
        opt = torch.optim.Adam(params, lr=1e-3, weight_decay=1e-7, fused=True, capturable=bool(args.graph))
        step = TrainStep(fwd, inputs, labels, loss_fn, opt, params, all_reduce=bool(args.graph or args.flat_params),
                         amp_dtype=amp_dtype, max_grad_norm=5.0, pre_step=pre_step, overlap_all_reduce=overlap,
                         force_collectives=FORCE_PG)
    else:
        step = FwdStep(model, inputs, pre_step)
    # --dump-outputs: the initial parameters, for the one reproducible step after the timed region
    first_step, snap = step, ([p.detach().clone() for p in step_params(step)] if args.dump_outputs else None)
    t_w = time.perf_counter()

    def first(i):
        torch.cuda.synchronize()  # (a progress line per warm-up step: a long MIOpen search is not a hang)
        log(f"[rank {rank}] warm-up step {i + 1} done at {time.perf_counter() - t_w:.1f} s")

    sync = None
    fell_back = None
    if args.graph:
        # eager warm-up on a side stream (MIOpen find, optimizer state), capture, 2 untimed replays.
        # The capture's outcome is agreed by all ranks before any replay (parallel.capture_collectively):
        # if the collectives inside one rank's capture failed, EVERY rank takes the serial all-reduce.
        def serial_step():
            torch.cuda.synchronize()
            flat_s = FlatParams(model, cast_dtype=amp_dtype)
            opt_s = torch.optim.Adam([flat_s.master], lr=1e-3, weight_decay=1e-7, fused=True, capturable=True)
            return TrainStep(flat_s.bind(model), inputs, labels, loss_fn, opt_s, [flat_s.master], all_reduce=True,
                             amp_dtype=amp_dtype, max_grad_norm=5.0, pre_step=pre_step, force_collectives=FORCE_PG)
        overlapped = args.mode == "train" and getattr(step, "overlap", False)
        fail = os.environ.get("LSS_BENCH_FAIL_CAPTURE_RANK", "") == str(rank)  # rehearsal of the fallback
        step, fell_back = parallel.capture_collectively(step, max(args.warmup, 2),
                                                        serial_step if overlapped else None, first, fail)
        if fell_back:
            log(f"[rank {rank}] every rank falls back to the serial all-reduce ({fell_back})")
        for _ in range(2):
            step()
        if args.mode == "train" and world > 1:
            # the replicas must be bit-identical after the updates (train_simbev.py:245-248): checksums
            # of every master gathered over the control group
            ok = parallel.replicas_in_sync(step.params)
            if not ok and getattr(step, "overlap", False):
                log(f"[rank {rank}] replicas differ after the overlapped captured all-reduce: re-broadcasting "
                    "rank 0's parameters, serial all-reduce")
                parallel.broadcast_state(model)
                step = parallel.recapture_collectively(serial_step, "replicas differed")
                for _ in range(2):
                    step()
                fell_back = "replicas differed after the overlapped captured all-reduce"
                ok = parallel.replicas_in_sync(step.params)
            if not ok:
                log(f"[rank {rank}] replicas differ after the untimed replays; not reporting a number")
                sys.exit(4)
            sync = {"checked": "checksums of every fp32 master, all ranks", "after_warmup": ok}
    else:
        for i in range(args.warmup):
            step()
            first(i)
    torch.cuda.synchronize()
    log(f"[rank {rank}] warmup {args.warmup} steps in {time.perf_counter() - t_w:.1f} s"
        + (" (incl. graph capture)" if args.graph else ""))

    ops.SPLAT_PROFILE.reset(False)
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if args.dump_outputs:
        # The timed path, called once more after the timed steps (every rank: its collectives) from the
        # run's initial state, so that its outputs are the same from run to run (restore_initial); a
        # forward-only step has no state and its last timed call is taken as it is.
        if snap:
            if step is first_step:
                restore_initial(step, snap, 1234 + rank)
            else:
                log(f"[rank {rank}] the step was rebuilt after a failed capture: outputs dumped from the trained state")
            out = step()
            torch.cuda.synchronize()
        if rank == 0:
            write_outputs(collect_outputs(step, out, args.mode), args.dump_outputs)
    splat_ms = None
    if args.full:
        # the splat kernel alone, kernel-stamped events (hipExtLaunchKernel) on eager steps after the
        # timed region, same inputs (a captured launch cannot carry kernel-stamped events)
        step.eager()  # the first eager step after the replays runs cold: not timed
        torch.cuda.synchronize()
        ops.SPLAT_PROFILE.reset(True)
        for _ in range(args.profile_steps):
            step.eager()
        torch.cuda.synchronize()
        ops.SPLAT_PROFILE.enabled = False
        splat_ms = ops.SPLAT_PROFILE.avg_ms()
        ops.SPLAT_PROFILE.release()
    per_rank_ms = [1e3 * elapsed / args.steps]
    if world > 1:
        t = torch.tensor([elapsed], device=dev)
        allt = [torch.zeros_like(t) for _ in range(world)]
        dist.all_gather(allt, t)
        per_rank_ms = [1e3 * float(x.item()) / args.steps for x in allt]
        elapsed = max(float(x.item()) for x in allt)
    log(f"[rank {rank}] {args.steps} steps in {elapsed:.3f} s, out {float(out.detach().float().mean()):.4f}")
    invalid = None
    if sync is not None:
        sync["after_timed"] = parallel.replicas_in_sync(step.params)
        if not sync["after_timed"]:
            # the same policy as after the warm-up: replicas that drifted apart during the timed
            # replays void the number (the line is printed marked invalid, then every rank exits 4)
            invalid = "replicas differ after the timed replays"
            log(f"[rank {rank}] {invalid}")

    if rank == 0:
        D, H, W = model.frustum.shape[:3]
        frames = world * B * args.steps
        what = "full train step (fwd+loss+bwd+clip+Adam)" if args.mode == "train" else "forward only"
        res = {
            "metric": METRIC, "value": round(frames / elapsed, 3), "unit": "frames/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(1e3 * elapsed / args.steps, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": args.dtype,
            "data": "synthetic (SimBEV-shaped rig, random-init weights)",
            "config": {"workload": f"{args.config}: B={B}/GPU x {N} cams x {fd[0]}x{fd[1]}, D={D}, {X}x{Y} BEV, "
                                   + what,
                       "global_batch": world * B, "parallelism": f"dp{world}", "bev_layout": args.bev_layout,
                       "inverse": "host torch.inverse", "fuse_depthnet": bool(args.fuse_depthnet),
                       "depthwise": args.dw_impl, "batchnorm": "hip" if args.hip_bn else "miopen",
                       "step": ("train_simbev.py loop, unchanged (eager, torch Adam, host inverse per forward)"
                                if args.caller == "reference" else "hipgraph" if args.graph else "eager"),
                       "flat_params": bool(args.flat_params),
                       "param_groups": bool(args.flat_params and args.param_groups),
                       "all_reduce": ("overlapped with backward (3 groups, captured)" if getattr(step, "overlap", False)
                                      else "one flat all-reduce between the graphs" if (world > 1 or FORCE_PG)
                                      else None)},
            "per_rank_ms_per_step": [round(x, 3) for x in per_rank_ms],
            "replicas_in_sync": sync, "capture_fallback": fell_back, "invalid": invalid,
        }
    if rank == 0 and args.full:
        with torch.no_grad():
            plan = model.plan(rig["rots"], rig["trans"], rig["intrins"], rig["post_rots"], rig["post_trans"])
            kept = int(plan.cell_start[-1].item())
            occupied = int((plan.cell_start[1:] > plan.cell_start[:-1]).sum().item())
        out_bytes = 2 if amp_dtype is not None else 4
        nbytes = splat_fwd_bytes(B, N, D, H, W, X, Y, Z, kept, out_bytes, ctx_bytes=out_bytes)
        nbytes_8d = splat_fwd_bytes_survey(B, N, D, H, W, X, Y, Z, out_bytes, out_bytes)
        # graded: the splat inside the timed graph replays when measured, else the eager stamped launches
        graded_us = in_graph["us"] if in_graph else (splat_ms * 1e3 if splat_ms else None)
        achieved = nbytes / (graded_us * 1e3) if graded_us else None
        roofline_bwd = None
        if args.mode == "train":
            bb = splat_bwd_bytes(B, N, D, H, W, occupied, out_bytes, out_bytes)
            ib = (in_graph or {}).get("bwd")
            roofline_bwd = {
                "kernel": "lss_splat_bwd (k_splat_bwd_tile)", "bound": "hbm", "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "algorithmic_bytes": bb["hbm"], "bytes_detail": bb, "gather_bytes_l2": kept * 64 * out_bytes,
                "us": ib["us"] if ib else None, "min_us": ib["min_us"] if ib else None,
                "achieved": round(bb["hbm"] / (ib["us"] * 1e3), 1) if ib else None,
                "frac": round(bb["hbm"] / (ib["us"] * 1e3) / HBM_PEAK_GBS, 4) if ib else None,
                "timed_in": "the captured step's graph replays (rocprofv3 --kernel-trace child, as roofline.in_graph)"}
        ceiling = write_ceiling(B * Z * 64 * X * Y, amp_dtype or torch.float32, dev)
        res.update({
            "roofline": {"kernel": "lss_splat_fwd", "bound": "hbm",
                         "graded": "frac: the kernel inside the timed region's graph replays (rocprofv3 --kernel-trace "
                                   "child of this script); eager_ext_events: eager launches with kernel-stamped "
                                   "hipEvents (hipExtLaunchKernel), which start 6 of the 8 XCDs ~1.1 us late",
                         "achieved": round(achieved, 1) if achieved else None, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": round(achieved / HBM_PEAK_GBS, 4) if achieved else None,
                         "traffic": traffic["hbm_bytes_per_launch"] if traffic else None,
                         "traffic_detail": traffic, "algorithmic_bytes": nbytes,
                         "algorithmic_bytes_survey_8d": nbytes_8d,
                         "frac_survey_8d": round(nbytes_8d / (graded_us * 1e3) / HBM_PEAK_GBS, 4) if graded_us else None,
                         "avg_launch_us": round(graded_us, 2) if graded_us else None,
                         "timed_in": ("the timed graph replays: rocprofv3 --kernel-trace (CP timestamps) of a child run "
                                      "of this script, same configuration" if in_graph else
                                      "eager steps after the timed region, kernel-stamped hipEvents"),
                         "in_graph": {**{k: v for k, v in in_graph.items() if k != "bwd"},
                                      "frac": round(nbytes / (in_graph["us"] * 1e3) / HBM_PEAK_GBS, 4),
                                      "frac_survey_8d": round(nbytes_8d / (in_graph["us"] * 1e3) / HBM_PEAK_GBS, 4)}
                                     if in_graph else None,
                         "eager_ext_events": {
                             "avg_launch_us": round(splat_ms * 1e3, 2),
                             "frac": round(nbytes / (splat_ms * 1e6) / HBM_PEAK_GBS, 4),
                             "frac_survey_8d": round(nbytes_8d / (splat_ms * 1e6) / HBM_PEAK_GBS, 4),
                             "note": "hipExtLaunchKernel with start/stop events: XCDs 2-7 start ~1.1 us after XCDs 0-1 "
                                     "(a plain launch or a graph replay starts all eight together: "
                                     "profiles/r06/xcd_start_probe.txt), so this reading includes that skew"}
                         if splat_ms else None,
                         "write_ceiling": dict(ceiling, splat_frac_of_ceiling=round(achieved / ceiling["GB/s"], 4)
                                               if achieved else None)},
            "roofline_bwd": roofline_bwd,
        })
        if args.cpu_baseline and world == 1 and args.config == "c3":
            log("[rank 0] timing the CPU baseline ...")
            t_c = time.perf_counter()
            res["cpu_baseline"] = cpu_baseline(model, args)
            log(f"[rank 0] CPU baseline in {time.perf_counter() - t_c:.1f} s")
        else:
            res["cpu_baseline"] = None
    if rank == 0:
        os.write(result_fd, (json.dumps(res) + "\n").encode())
    if world > 1 or FORCE_PG:
        dist.destroy_process_group()
    watchdog.cancel()
    if invalid:
        sys.exit(4)


if __name__ == "__main__":
    main()
