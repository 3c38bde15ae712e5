"""Squeeze-excite time per MBConv block from two rocprofv3 kernel traces of bench.py (graph replays).

usage: python scripts/se_per_shape.py <fallback_kernel_trace.csv> <tails_kernel_trace.csv> [first_step last_step]
Steps are delimited by k_geometry_cells, as in step_kernels.py. Within a step the i-th forward reduction
(k_se_mean*) belongs to MBConv block i and the i-th backward reduction (k_se_dot*) to block 15 - i; the MLP
kernels that follow a reduction, up to the streaming pass (k_se_scale / k_se_dx), are charged to it. Prints,
per block, the reduction's grid in the second trace (blocks x threads), the average us of reduction + MLP
in both traces, and the k_se_* totals per step.
"""
import csv
import sys


def load(path, s0, s1):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    geo = [i for i, r in enumerate(rows) if "k_geometry_cells" in r["Kernel_Name"]]
    n = s1 - s0
    fwd, bwd, total, launches = {}, {}, 0.0, 0
    for s in range(s0, s1):
        cur, idx = None, {"f": 0, "b": 0}
        for r in rows[geo[s]:geo[s + 1]]:
            k = r["Kernel_Name"]
            if "k_se_" not in k:
                continue
            d = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
            total += d
            launches += 1
            if "k_se_mean" in k or "k_se_dot" in k:
                side = "f" if "k_se_mean" in k else "b"
                grid = f'{int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"])}x{r["Workgroup_Size_X"]}'  # blocks x threads
                cur = (fwd if side == "f" else bwd).setdefault(idx[side], [0.0, grid])
                idx[side] += 1
                cur[0] += d
            elif "k_se_mlp" in k and cur is not None:
                cur[0] += d
            else:
                cur = None
    return ({i: (v[0] / n, v[1]) for i, v in fwd.items()}, {i: (v[0] / n, v[1]) for i, v in bwd.items()},
            total / n, launches / n)


def main():
    s0 = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    s1 = int(sys.argv[4]) if len(sys.argv) > 4 else 23
    a, b = load(sys.argv[1], s0, s1), load(sys.argv[2], s0, s1)
    print(f"steps {s0}..{s1}; k_se_* per step: fallback {a[2]:.1f} us in {a[3]:.0f} launches, "
          f"tails {b[2]:.1f} us in {b[3]:.0f} launches")
    for name, fa, fb, blk in (("forward  mean + mlp1 + mlp2 -> mean_tail", a[0], b[0], lambda i: i),
                              ("backward dot + mlpb1 + mlpb2 -> dot_tail", a[1], b[1], lambda i: len(a[1]) - 1 - i)):
        print(f"{name}\n  block  grid (2nd trace)  fallback us   tails us   saved")
        for i in sorted(fa):
            print(f"  {blk(i):5d} {fb[i][1]:>16s} {fa[i][0]:12.2f} {fb[i][0]:10.2f} {fa[i][0] - fb[i][0]:7.2f}"
                  + ("   <-- slower" if fb[i][0] >= fa[i][0] else ""))
        print(f"  sum                    {sum(v[0] for v in fa.values()):12.2f} {sum(v[0] for v in fb.values()):10.2f}")


if __name__ == "__main__":
    main()
