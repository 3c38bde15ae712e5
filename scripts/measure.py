"""One parameterised GPU measurement runner (replaces the one-shot gpu_r4_* / gpu_r5_* scripts).

Runs the steps given on the command line in order, each under its own time limit, and stops at the
first step that fails (no retries). Outputs go to gpurun_out/<tag>/; copy what should be judged into
profiles/rNN/ (scripts/README.md lists which profile came from which step).

  python scripts/measure.py --tag r6a tests smoke "bench:c3" "trace:c3" \
      "bench:c3_caller:--caller reference --cpu-baseline 0 --pmc-traffic 0" \
      "pmc:plan:TCC_EA0_RDREQ_sum TCC_EA0_WRREQ_sum:k_scan|k_scatter|k_csr|k_geometry:--graph 0"

Steps:
  tests[:pytest args]                 GPU suite (one process), log + summary line
  smoke                               __graft_entry__.smoke()
  bench:NAME[:bench.py args]          bench.py --full, its JSON line kept as NAME.json
  trace:NAME[:bench.py args]          rocprofv3 --kernel-trace --stats of bench.py --full (20 timed replays):
                                      NAME_kernel_stats.csv, NAME_hot_steps.txt, NAME_step_kernels.txt,
                                      NAME_steady_summary.json
  pmc:NAME:COUNTERS:REGEX[:args]      one rocprofv3 --pmc pass (COUNTERS space-separated, one block's
                                      limits) over bench.py (eager steps) for kernels matching REGEX:
                                      per-kernel averages in NAME.txt
  kbench:NAME:args                    scripts/kbench.py with args, log kept
  py:NAME:script args                 python scripts/<script> args (a diagnostics script), log kept
  train_loop[:steps]                  trainer.train on a synthetic SimBEV tree at config-3 sizes (224x480 JPEGs, B=8,
                                      written to a temporary directory): frames/s of (a) the loop with 14 loader
                                      workers, (b) the loop cycling pre-decoded host batches, (c) bench.py's default,
                                      (d) bench.py --caller reference, in train_loop.json
  train_loop_bev[:steps[:runs]]       the same tree and the same two loops with the BEV-space augmentation off and on
                                      (--bev-rot-lim=-22.5,22.5 --bev-scale-lim 0.9,1.1 --bev-flip 1) alternately, RUNS (3)
                                      fresh processes each: train_loop_bev.json
  photo[:steps[:runs[:PARENT_LIB]]]   the photometric augmentation: scripts/photo_bench.py (lss_simbev_images against
                                      lss_simbev_images_photo at the staging shape, neutral / colour / colour + noise records,
                                      graph replays; PARENT_LIB: the parent commit's library, its plain kernel as the base):
                                      photo_kernel.json; then the same tree and the two loops of train_loop_bev with
                                      --photo 0 and --photo 1 alternately, RUNS (3) fresh processes each: train_loop_photo.json
  infer[:PARENT_DIR]                  the eval-mode forward with and without the lss_bn_eval path: bench.py --config c2
                                      on a checkout of the parent commit (PARENT_DIR, library built there) and on this
                                      tree alternately, three runs each, and --hip-bn 0 here; scripts/infer_ab.py (the
                                      Predictor at c3 sizes, norm.USE_HIP_BN_EVAL on / off alternately, bsz 8 and 1); the
                                      default training line on each side; kernel traces of the Predictor, switch on and
                                      off, in runs of their own: infer.json, infer_kernels.txt
  bench_ab:PARENT_DIR[:RUNS]          the default ``python bench.py`` line on a checkout of the parent commit (library built
                                      there) and on this tree alternately, RUNS (3) each: bench_parent_<i>.json,
                                      bench_this_<i>.json, bench_ab.txt
  lib:VARIANT                         later steps load lss-carla_amd/variants/VARIANT.so (product: the default)
"""
from __future__ import annotations

import argparse
import collections
import csv
import glob
import os
import re
import shlex
import shutil
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PY = sys.executable


def run(cmd, log_path, limit, env=None, cwd=REPO) -> int:
    """cmd under `timeout -k 10 limit`, stdout+stderr to log_path; prints a progress line."""
    t0 = time.time()
    full = ["timeout", "-k", "10", str(limit)] + cmd
    with open(log_path, "w") as fh:
        proc = subprocess.Popen(full, stdout=fh, stderr=subprocess.STDOUT, env=env, cwd=cwd)
        while True:  # a heartbeat: a first step compiling library kernels can be silent for minutes
            try:
                rc = proc.wait(timeout=50)
                break
            except subprocess.TimeoutExpired:
                print(f"  ... {os.path.basename(log_path)} running, {time.time() - t0:.0f} s", flush=True)
    print(f"  rc={rc} in {time.time() - t0:.0f} s ({os.path.basename(log_path)})", flush=True)
    return rc


def tail(path, n=3) -> str:
    try:
        with open(path, errors="replace") as fh:
            return "".join(fh.readlines()[-n:])
    except OSError:
        return ""


def prof_env():
    return dict(os.environ, TMPDIR="/tmp")


def bench_args(extra: str) -> list:
    return shlex.split(extra) if extra else []


def step_tests(out, spec):
    args = shlex.split(spec) if spec else []
    if not any(a.startswith("tests") for a in args):
        args = ["tests"] + args
    log = os.path.join(out, "gpu_tests.log")
    rc = run([PY, "-u", "-m", "pytest", "-m", "gpu", "-q", "-rs", "-p", "no:cacheprovider",
              "--timeout", "200", "--timeout-method", "thread"] + args, log, 1000)
    print(tail(log, 3), flush=True)
    return rc


def step_smoke(out, _):
    log = os.path.join(out, "smoke.log")
    rc = run([PY, "-u", "-c", "import __graft_entry__ as g; g.smoke()"], log, 300)
    print(tail(log, 1), flush=True)
    return rc


def step_bench(out, spec):
    name, _, extra = spec.partition(":")
    log = os.path.join(out, f"{name}.log")
    rc = run([PY, "-u", "bench.py", "--full"] + bench_args(extra), log, 1000)
    last = tail(log, 1).strip()
    if rc == 0 and last.startswith("{"):
        with open(os.path.join(out, f"{name}.json"), "w") as fh:
            fh.write(last + "\n")
        print(last[:400], flush=True)
    else:
        print(tail(log, 15), flush=True)
    return rc


def step_trace(out, spec):
    name, _, extra = spec.partition(":")
    d = f"/tmp/measure_trace_{name}"
    shutil.rmtree(d, ignore_errors=True)
    log = os.path.join(out, f"{name}_trace.log")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "run", "--",
           PY, "-u", os.path.join(REPO, "bench.py"), "--full", "--steps", "20", "--warmup", "3",
           "--profile-steps", "0", "--cpu-baseline", "0", "--pmc-traffic", "0", "--in-graph-prof", "0"] \
        + bench_args(extra)
    rc = run(cmd, log, 700, env=prof_env(), cwd="/tmp")
    if rc != 0:
        print(tail(log, 15), flush=True)
        return rc
    tr = (glob.glob(f"{d}/**/run_kernel_trace.csv", recursive=True) or [None])[0]
    st = (glob.glob(f"{d}/**/run_kernel_stats.csv", recursive=True) or [None])[0]
    if st:
        shutil.copy(st, os.path.join(out, f"{name}_kernel_stats.csv"))
    if tr:
        for script, suffix, args in (("hot_steps.py", "hot_steps.txt", ["5", "23"]),
                                     ("step_kernels.py", "step_kernels.txt", ["5", "23", "400"]),
                                     ("steady_summary.py", "steady_summary.json", [])):
            with open(os.path.join(out, f"{name}_{suffix}"), "w") as fh:
                subprocess.call([PY, os.path.join(REPO, "scripts", script), tr] + args, stdout=fh,
                                stderr=subprocess.STDOUT)
        keep = os.path.join(out, f"{name}_kernel_trace.csv")
        # gpurun copies back at most 64 MiB of gpurun_out/: keep a trace only while the tag stays < 40 MiB
        used = sum(os.path.getsize(os.path.join(out, f)) for f in os.listdir(out))
        if used + os.path.getsize(tr) < 40 << 20:
            shutil.copy(tr, keep)
        print(tail(os.path.join(out, f"{name}_hot_steps.txt"), 12), flush=True)
    shutil.rmtree(d, ignore_errors=True)
    return 0


def step_pmc(out, spec):
    name, counters, regex, *rest = spec.split(":", 3)
    extra = rest[0] if rest else ""
    d = f"/tmp/measure_pmc_{name}"
    shutil.rmtree(d, ignore_errors=True)
    log = os.path.join(out, f"{name}_pmc.log")
    cmd = (["timeout", "-s", "KILL", "240", "rocprofv3", "--pmc"] + counters.split()
           + ["--output-format", "csv", "-d", d, "-o", "run", "--", PY, "-u", os.path.join(REPO, "bench.py"),
              "--full", "--steps", "6", "--warmup", "3", "--profile-steps", "0", "--graph", "0", "--cpu-baseline", "0",
              "--pmc-traffic", "0", "--in-graph-prof", "0"] + bench_args(extra))
    rc = run(cmd, log, 260, env=prof_env(), cwd="/tmp")
    if rc != 0:
        print(tail(log, 10), flush=True)
        return rc
    pat = re.compile(regex)
    vals = collections.defaultdict(lambda: collections.defaultdict(list))
    files = glob.glob(f"{d}/**/*counter_collection.csv", recursive=True)
    if files and os.path.getsize(files[0]) < 32 << 20:  # kept for scripts/step_roofline.py
        shutil.copy(files[0], os.path.join(out, f"{name}_counter_collection.csv"))
    for f in files:
        for r in csv.DictReader(open(f)):
            k = r["Kernel_Name"]
            if pat.search(k):
                key = re.sub(r"\(anonymous namespace\)::", "", k).split("(")[0][:70]
                vals[key][r["Counter_Name"]].append(float(r["Counter_Value"]))
    with open(os.path.join(out, f"{name}.txt"), "w") as fh:
        fh.write(f"# rocprofv3 --pmc {counters} over bench.py --graph 0 {extra}; per-dispatch averages "
                 f"(first 2 dispatches of each kernel dropped)\n")
        for k, dd in sorted(vals.items()):
            fh.write(k + "\n")
            for c in sorted(dd):
                v = dd[c][2:] if len(dd[c]) > 4 else dd[c]
                fh.write(f"   {c:28s} {sum(v) / len(v):16.1f}   (n={len(v)})\n")
    print(open(os.path.join(out, f"{name}.txt")).read()[:3000], flush=True)
    shutil.rmtree(d, ignore_errors=True)
    return 0


def step_kbench(out, spec):
    name, _, extra = spec.partition(":")
    log = os.path.join(out, f"{name}.log")
    rc = run([PY, "-u", os.path.join("scripts", "kbench.py")] + bench_args(extra), log, 600)
    print(tail(log, 25), flush=True)
    return rc


def step_py(out, spec):
    name, _, extra = spec.partition(":")
    args = shlex.split(extra)
    log = os.path.join(out, f"{name}.log")
    rc = run([PY, "-u", os.path.join("scripts", args[0])] + args[1:], log, 600)
    print(tail(log, 40), flush=True)
    return rc


def step_train_loop(out, spec):
    import json
    import tempfile
    steps = int(spec) if spec else 200
    script = os.path.join("scripts", "train_loop.py")
    result = {"steps": steps, "bsz": 8}

    def last_json(log):
        last = tail(log, 1).strip()
        return json.loads(last) if last.startswith("{") else None

    with tempfile.TemporaryDirectory(prefix="lss_simbev_") as root:
        # 80 % of the samples train: enough for `steps` batches of 8 in one epoch
        samples = int(steps * 8 / 0.8) + 40
        rc = run([PY, "-u", script, "--make", root, "--samples", str(samples)], os.path.join(out, "tree.log"), 900)
        if rc != 0:
            return rc
        for key, extra in (("a_loop_14_workers", ["--nworkers", "14"]),
                           ("b_loop_predecoded", ["--nworkers", "0", "--cycle-batches", "4"])):
            log = os.path.join(out, f"train_loop_{key}.log")
            rc = run([PY, "-u", script, "--dataroot", root, "--steps", str(steps)] + extra, log, 900)
            got = last_json(log) if rc == 0 else None
            if got is None:
                print(tail(log, 15), flush=True)
                return rc or 1
            result[key] = got["frames_per_s"]
            print(f"  {key}: {got}", flush=True)
    for key, extra in (("c_bench_default", []), ("d_bench_reference_caller", ["--caller", "reference"])):
        log = os.path.join(out, f"train_loop_{key}.log")
        rc = run([PY, "-u", "bench.py", "--gpus", "1"] + extra, log, 900)
        got = last_json(log) if rc == 0 else None
        if got is None:
            print(tail(log, 15), flush=True)
            return rc or 1
        result[key] = got.get("value")
        print(f"  {key}: {got.get('value')} {got.get('unit', '')}", flush=True)
    with open(os.path.join(out, "train_loop.json"), "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result), flush=True)
    return 0


def step_train_loop_bev(out, spec):
    import json
    import tempfile
    steps, _, runs = spec.partition(":")
    steps, runs = int(steps or 200), int(runs or 3)
    script = os.path.join("scripts", "train_loop.py")
    on = ["--bev-rot-lim=-22.5,22.5", "--bev-scale-lim", "0.9,1.1", "--bev-flip", "1"]
    loops = (("loop_14_workers", ["--nworkers", "14"]), ("loop_predecoded", ["--nworkers", "0", "--cycle-batches", "4"]))
    result = {"steps": steps, "bsz": 8, "runs": runs, **{k: {"off": [], "on": []} for k, _ in loops}}
    with tempfile.TemporaryDirectory(prefix="lss_simbev_") as root:
        samples = int(steps * 8 / 0.8) + 40
        rc = run([PY, "-u", script, "--make", root, "--samples", str(samples)], os.path.join(out, "tree.log"), 900)
        if rc != 0:
            return rc
        for key, extra in loops:
            for i in range(1, runs + 1):
                for side, aug in (("off", []), ("on", on)):
                    log = os.path.join(out, f"train_loop_bev_{key}_{side}_{i}.log")
                    rc = run([PY, "-u", script, "--dataroot", root, "--steps", str(steps)] + extra + aug, log, 600)
                    last = tail(log, 1).strip()
                    if rc != 0 or not last.startswith("{"):
                        print(tail(log, 15), flush=True)
                        return rc or 1
                    got = json.loads(last)
                    if got["skipped"]:
                        print(f"  {key} {side} {i}: {got['skipped']} skipped steps", flush=True)
                        return 1
                    result[key][side].append(got["frames_per_s"])
                    print(f"  {key} {side} {i}: {got['frames_per_s']:.1f} frames/s", flush=True)
    with open(os.path.join(out, "train_loop_bev.json"), "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result), flush=True)
    return 0


def step_photo(out, spec):
    import json
    import tempfile
    parts = spec.split(":") if spec else []
    steps, runs = int(parts[0]) if parts and parts[0] else 200, int(parts[1]) if len(parts) > 1 and parts[1] else 3
    parent_lib = os.path.abspath(parts[2]) if len(parts) > 2 and parts[2] else None
    log = os.path.join(out, "photo_kernel.log")
    rc = run([PY, "-u", os.path.join("scripts", "photo_bench.py")] + (["--parent-lib", parent_lib] if parent_lib else []),
             log, 300)
    last = tail(log, 1).strip()
    if rc != 0 or not last.startswith("{"):
        print(tail(log, 15), flush=True)
        return rc or 1
    with open(os.path.join(out, "photo_kernel.json"), "w") as fh:
        json.dump(json.loads(last), fh, indent=1)
        fh.write("\n")
    print(last, flush=True)
    if steps <= 0:
        return 0
    script = os.path.join("scripts", "train_loop.py")
    loops = (("loop_14_workers", ["--nworkers", "14"]), ("loop_predecoded", ["--nworkers", "0", "--cycle-batches", "4"]))
    result = {"steps": steps, "bsz": 8, "runs": runs, **{k: {"off": [], "on": []} for k, _ in loops}}
    with tempfile.TemporaryDirectory(prefix="lss_simbev_") as root:
        samples = int(steps * 8 / 0.8) + 40
        rc = run([PY, "-u", script, "--make", root, "--samples", str(samples)], os.path.join(out, "tree.log"), 900)
        if rc != 0:
            return rc
        for key, extra in loops:
            for i in range(1, runs + 1):
                for side, aug in (("off", []), ("on", ["--photo", "1"])):
                    log = os.path.join(out, f"train_loop_photo_{key}_{side}_{i}.log")
                    rc = run([PY, "-u", script, "--dataroot", root, "--steps", str(steps)] + extra + aug, log, 600)
                    last = tail(log, 1).strip()
                    if rc != 0 or not last.startswith("{"):
                        print(tail(log, 15), flush=True)
                        return rc or 1
                    got = json.loads(last)
                    if got["skipped"]:
                        print(f"  {key} {side} {i}: {got['skipped']} skipped steps", flush=True)
                        return 1
                    result[key][side].append(got["frames_per_s"])
                    print(f"  {key} {side} {i}: {got['frames_per_s']:.1f} frames/s", flush=True)
    with open(os.path.join(out, "train_loop_photo.json"), "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result), flush=True)
    return 0


def _bench_value(cmd, log, cwd, limit=600):
    import json
    rc = run(cmd, log, limit, cwd=cwd)
    last = tail(log, 1).strip()
    if rc != 0 or not last.startswith("{"):
        print(tail(log, 15), flush=True)
        return rc or 1, None
    got = json.loads(last)
    return 0, {"value": got.get("value"), "unit": got.get("unit"), "ms_per_step": got.get("ms_per_step")}


def step_infer(out, spec):
    """infer:PARENT_DIR -- the eval-mode forward before and after the lss_bn_eval path, in one session: bench.py
    --config c2 (fp32 forward, the project's own line) on a checkout of the parent commit (PARENT_DIR, with its own
    build of the library) and on this tree alternately, three runs each, and --hip-bn 0 on this tree; the Predictor
    at c3 sizes with norm.USE_HIP_BN_EVAL on / off alternately (scripts/infer_ab.py, bsz 8 and 1); the default
    training line once on each side; then rocprofv3 --kernel-trace --stats runs of their own, switch on and off.
    Writes infer.json and infer_kernels.txt."""
    import json
    parent = os.path.abspath(spec) if spec else None
    result = {"c2": {"parent": [], "this": []}, "predictor": {}, "train_default": {}}
    sides = ([("parent", parent)] if parent else []) + [("this", REPO)]
    for i in range(3):
        for side, cwd in sides:
            rc, got = _bench_value([PY, "-u", "bench.py", "--config", "c2"], os.path.join(out, f"c2_{side}_{i}.log"), cwd)
            if rc != 0:
                return rc
            result["c2"][side].append(got)
            print(f"  c2 {side} {i}: {got}", flush=True)
    rc, got = _bench_value([PY, "-u", "bench.py", "--config", "c2", "--hip-bn", "0"], os.path.join(out, "c2_hip_bn_0.log"), REPO)
    if rc != 0:
        return rc
    result["c2"]["this_hip_bn_0"] = got
    print(f"  c2 this --hip-bn 0: {got}", flush=True)
    for bsz in (8, 1):
        log = os.path.join(out, f"predictor_bsz{bsz}.log")
        rc = run([PY, "-u", os.path.join("scripts", "infer_ab.py"), "--bsz", str(bsz), "--frames", "400", "--legs", "3"],
                 log, 600)
        last = tail(log, 1).strip()
        if rc != 0 or not last.startswith("{"):
            print(tail(log, 15), flush=True)
            return rc or 1
        result["predictor"][f"bsz{bsz}"] = json.loads(last)
        print(f"  predictor bsz {bsz}: {last}", flush=True)
    for side, cwd in sides:
        rc, got = _bench_value([PY, "-u", "bench.py"], os.path.join(out, f"train_{side}.log"), cwd)
        if rc != 0:
            return rc
        result["train_default"][side] = got
        print(f"  default training line, {side}: {got}", flush=True)
    # kernel traces, each in a run of its own: launches and time per forward by kernel class
    replays = 20
    classes = (("k_bn_eval*", re.compile(r"k_bn_eval")), ("stock batch norm", re.compile(r"(?i)batch_?norm|BatchNorm")),
               ("elementwise", re.compile(r"(?i)elementwise")), ("everything else", re.compile(r"")))
    n = replays + 2
    lines = [f"# rocprofv3 --kernel-trace --stats over scripts/infer_ab.py --bsz 8 --only on|off --calls {replays}: one eager "
             f"warm-up forward, the first call's replay and {replays} more = {n} forwards (plus the Predictor's construction "
             f"and the input copies of each call: a few launches); per forward = totals / {n}"]
    result["kernels"] = {}
    for sw in ("on", "off"):
        d = f"/tmp/measure_infer_{sw}"
        shutil.rmtree(d, ignore_errors=True)
        rc = run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "run", "--", PY, "-u",
                  os.path.join(REPO, "scripts", "infer_ab.py"), "--bsz", "8", "--only", sw, "--calls", str(replays)],
                 os.path.join(out, f"trace_{sw}.log"), 600, env=prof_env(), cwd="/tmp")
        st = (glob.glob(f"{d}/**/run_kernel_stats.csv", recursive=True) or [None])[0]
        if rc != 0 or not st:
            print(tail(os.path.join(out, f"trace_{sw}.log"), 15), flush=True)
            return rc or 1
        shutil.copy(st, os.path.join(out, f"infer_{sw}_kernel_stats.csv"))
        tot = collections.OrderedDict((name, [0, 0.0]) for name, _ in classes)
        for r in csv.DictReader(open(st)):
            name = next(n for n, pat in classes if pat.search(r["Name"]))
            tot[name][0] += int(r["Calls"])
            tot[name][1] += float(r["TotalDurationNs"]) / 1e3
        lines.append(f"USE_HIP_BN_EVAL {sw}")
        result["kernels"][sw] = {}
        for name, (calls, us) in tot.items():
            lines.append(f"   {name:18s} {calls / n:8.1f} launches / forward   {us / n:10.1f} us / forward")
            result["kernels"][sw][name] = {"launches_per_forward": round(calls / n, 1), "us_per_forward": round(us / n, 1)}
        all_calls, all_us = sum(c for c, _ in tot.values()), sum(u for _, u in tot.values())
        lines.append(f"   {'total':18s} {all_calls / n:8.1f} launches / forward   {all_us / n:10.1f} us / forward")
        result["kernels"][sw]["total"] = {"launches_per_forward": round(all_calls / n, 1), "us_per_forward": round(all_us / n, 1)}
        shutil.rmtree(d, ignore_errors=True)
    with open(os.path.join(out, "infer_kernels.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    with open(os.path.join(out, "infer.json"), "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print("\n".join(lines), flush=True)
    return 0


def step_bench_ab(out, spec):
    """bench_ab:PARENT_DIR[:RUNS] -- the default ``python bench.py`` line on a checkout of the parent commit (PARENT_DIR,
    with its own build of the library) and on this tree alternately, RUNS (3) fresh processes each; every JSON line is
    kept as bench_parent_<i>.json / bench_this_<i>.json, and bench_ab.txt says whether this tree's runs lie inside the
    parent's run-to-run spread."""
    import json
    parent, _, runs = spec.partition(":")
    parent, runs = os.path.abspath(parent), int(runs or 3)
    vals = {"parent": [], "this": []}
    for i in range(1, runs + 1):
        for side, cwd in (("parent", parent), ("this", REPO)):
            log = os.path.join(out, f"bench_{side}_{i}.log")
            rc = run([PY, "-u", "bench.py"], log, 400, cwd=cwd)
            last = tail(log, 1).strip()
            if rc != 0 or not last.startswith("{"):
                print(tail(log, 15), flush=True)
                return rc or 1
            with open(os.path.join(out, f"bench_{side}_{i}.json"), "w") as fh:
                fh.write(last + "\n")
            got = json.loads(last)
            vals[side].append(got.get("value"))
            print(f"  {side} {i}: {got.get('value')} {got.get('unit', '')} ({got.get('ms_per_step')} ms / step)", flush=True)
    lo, hi = min(vals["parent"]), max(vals["parent"])
    inside = [lo <= v <= hi for v in vals["this"]]
    lines = [f"python bench.py, parent tree and this tree alternately, {runs} fresh processes each, one MI355X, one session",
             "parent: " + " ".join(f"{v:.3f}" for v in vals["parent"]) + f"   (spread {lo:.3f} - {hi:.3f})",
             "this:   " + " ".join(f"{v:.3f}" for v in vals["this"]),
             f"runs of this tree inside the parent's spread: {sum(inside)} of {len(inside)}"]
    with open(os.path.join(out, "bench_ab.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", required=True)
    ap.add_argument("steps", nargs="+")
    a = ap.parse_args()
    out = os.path.join(REPO, "gpurun_out", a.tag)
    os.makedirs(out, exist_ok=True)
    os.chdir(REPO)
    fns = {"tests": step_tests, "smoke": step_smoke, "bench": step_bench, "trace": step_trace, "pmc": step_pmc,
           "kbench": step_kbench, "py": step_py, "train_loop": step_train_loop, "train_loop_bev": step_train_loop_bev, "infer": step_infer, "bench_ab": step_bench_ab,
           "photo": step_photo}
    for s in a.steps:
        kind, _, spec = s.partition(":")
        print(f"== {s}", flush=True)
        if kind == "lib":
            if spec in ("", "product"):
                os.environ.pop("LSS_LIB", None)
            else:
                os.environ["LSS_LIB"] = os.path.join(REPO, "lss-carla_amd", "variants", spec + ".so")
            continue
        if kind == "env":  # env:NAME=VALUE for the steps that follow (env:NAME= unsets)
            k, _, v = spec.partition("=")
            if v:
                os.environ[k] = v
            else:
                os.environ.pop(k, None)
            continue
        rc = fns[kind](out, spec)
        if rc != 0:
            print(f"step {s!r} failed (rc={rc}); stopping", flush=True)
            sys.exit(rc if 0 < rc < 256 else 1)


if __name__ == "__main__":
    main()
