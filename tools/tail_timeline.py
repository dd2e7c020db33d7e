"""Per-launch table of the last matching pass of a rocprofv3 --kernel-trace run of the S200 step: python3 tools/tail_timeline.py <dir>
A pass starts with match_openprep_kernel; the n-th dispatch of a kernel behind it belongs to launch n. Per kernel and launch: start
(us from the first sweep's start), duration, hardware queue; then the gaps between the sweeps and the span of the pass."""
import csv, glob, sys
from collections import defaultdict

fn = sorted(glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True))[-1]
rows = sorted(csv.DictReader(open(fn)), key=lambda r: int(r["Start_Timestamp"]))


def short(r):
    n = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").replace("eacham::", "")
    return n.split("(")[0][:44]


preps = [i for i, r in enumerate(rows) if "match_openprep_kernel" in r["Kernel_Name"]]
which = int(sys.argv[2]) if len(sys.argv) > 2 else -1   # which pass of the run (default: the last)
a = preps[which]
b = preps[which + 1] if which != -1 and which + 1 < len(preps) else len(rows)
seg = [r for r in rows[a:b] if "match_" in r["Kernel_Name"] or "scan_counts" in r["Kernel_Name"] or "compact_edges" in r["Kernel_Name"]]
sweeps = [r for r in seg if "match_screen_kernel" in r["Kernel_Name"]]
t0 = int(sweeps[0]["Start_Timestamp"])
per = defaultdict(list)
order = []
for r in seg:
    n = short(r)
    if n not in per:
        order.append(n)
    per[n].append(r)
print(f"{fn}: pass {which} of {len(preps)}, {len(seg)} dispatches")
print(f"{'kernel':46s}" + "".join(f"{'launch ' + str(k + 1) + ': start / dur / q':>30s}" for k in range(len(sweeps))))
for n in order:
    cells = ""
    for r in per[n]:
        s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
        cells += f"{(s - t0) / 1e3:14.1f} {(e - s) / 1e3:9.1f} {r.get('Queue_Id', '?'):>5s}"
    print(f"{n:46s}{cells}")
ends = [int(r["End_Timestamp"]) for r in sweeps]
starts = [int(r["Start_Timestamp"]) for r in sweeps]
print("sweeps us        " + " / ".join(f"{(e - s) / 1e3:.1f}" for s, e in zip(starts, ends)))
print("gaps us          " + " / ".join(f"{(starts[k + 1] - ends[k]) / 1e3:.1f}" for k in range(len(sweeps) - 1)))
last = max(int(r["End_Timestamp"]) for r in seg)
print(f"last sweep's end to the last kernel's end {(last - ends[-1]) / 1e3:.1f} us; first sweep's start to the last kernel's end {(last - t0) / 1e3:.1f} us")
tail = [r for r in seg if not any(k in r["Kernel_Name"] for k in ("match_screen_kernel", "match_sweep_kernel", "match_openprep"))]
for k in range(len(sweeps)):
    mine = [per[n][k] for n in order if len(per[n]) > k and per[n][k] in tail]
    if mine:
        s = min(int(r["Start_Timestamp"]) for r in mine)
        e = max(int(r["End_Timestamp"]) for r in mine)
        print(f"tail of launch {k + 1}: {len(mine)} kernels, sum of durations {sum(int(r['End_Timestamp']) - int(r['Start_Timestamp']) for r in mine) / 1e3:.1f} us, "
              f"first start to last end {(e - s) / 1e3:.1f} us, from {(s - t0) / 1e3:.1f} to {(e - t0) / 1e3:.1f}")
