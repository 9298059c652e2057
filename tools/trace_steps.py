"""Per-kernel time over the LAST steps of a rocprofv3 --kernel-trace CSV (what ran before them — warm-up, a stand-in's training — is left out): calls and
microseconds per step for every kernel, the GPU's busy and idle time per step, and the wall time per step from anchor to anchor.
usage: python tools/trace_steps.py <kernel_trace.csv> [steps=40] [anchor-kernel-substring=planes_kernel]"""
import csv
import sys
from collections import defaultdict

rows = list(csv.DictReader(open(sys.argv[1])))
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 40
anchor = sys.argv[3] if len(sys.argv) > 3 else "planes_kernel"
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
idx = [i for i, r in enumerate(rows) if anchor in r["Kernel_Name"]]
if len(idx) < steps + 1:
    sys.exit(f"anchor kernel found {len(idx)} times, {steps + 1} needed")
a, b = idx[-steps - 1], idx[-1]
t0, t1 = int(rows[a]["Start_Timestamp"]), int(rows[b]["Start_Timestamp"])
per, calls = defaultdict(int), defaultdict(int)
busy_until, busy = t0, 0
for r in rows[a:b]:
    s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
    name = r["Kernel_Name"].replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "").replace("mnf::", "")[:72]
    per[name] += e - s
    calls[name] += 1
    if e > busy_until:
        busy += e - max(s, busy_until)
        busy_until = e
wall = (t1 - t0) / 1e3 / steps
print(f"last {steps} steps ({anchor} to {anchor}): {wall:.1f} us per step wall, GPU busy {busy / 1e3 / steps:.1f} us, idle {wall - busy / 1e3 / steps:.1f} us; "
      f"{(b - a) / steps:.1f} launches per step, kernel time summed {sum(per.values()) / 1e3 / steps:.1f} us")
for name, ns in sorted(per.items(), key=lambda kv: -kv[1]):
    print(f"{ns / 1e3 / steps:9.1f} us  {calls[name] / steps:6.2f} calls  {name}")
