#!/usr/bin/env python3
"""Per-kernel tables from the kernel trace of `MODE=trace tools/translate_bench.py`: the I/O kernels by launch shape, and the
large-frame translation next to the 12 x 256^2 one (the same pixel count), kernel by kernel, with the time per pixel of each.

    python tools/translate_trace_tables.py OUT/trace/tr_kernel_trace.csv"""
import collections
import csv
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
rows.sort(key=lambda r: int(r["Dispatch_Id"]))
def short(n):
    n = n.replace("void ", "")
    return n.split("(")[0]
ev = [(short(r["Kernel_Name"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3, (int(r["Grid_Size_X"]), int(r["Grid_Size_Y"]), int(r["Grid_Size_Z"]))) for r in rows]
# I/O kernels by grid
io = collections.defaultdict(list)
for n, us, g in ev:
    if n in ("k_image_load", "k_to_display_hw", "k_image_metrics", "k_metrics_final"):
        io[(n, g)].append(us)
for k, v in sorted(io.items()):
    v2 = sorted(v); print(k, "n=%d median %.2f us min %.2f max %.2f" % (len(v), v2[len(v2)//2], v2[0], v2[-1]))
# segments: find last k_metrics_final (end of io_pass(sq8) in the last iteration)
idx = [i for i, e in enumerate(ev) if e[0] == "k_metrics_final"]
last = idx[-1]
seg = ev[last + 1:]
# split at the to_display_hw that ends translate_images
cut = max(i for i, e in enumerate(seg) if e[0] == "k_to_display_hw")
bigs, sqs = seg[:cut + 1], seg[cut + 1:]
def table(s):
    t = collections.OrderedDict()
    for n, us, g in s:
        a = t.setdefault(n, [0, 0.0]); a[0] += 1; a[1] += us
    return t
tb, ts = table(bigs), table(sqs)
print("big total %.1f us (%d launches)   sq12 total %.1f us (%d launches)" % (sum(v[1] for v in tb.values()), len(bigs), sum(v[1] for v in ts.values()), len(sqs)))
print("%-34s %5s %9s %9s | %5s %9s %9s | ratio/px" % ("kernel", "n", "us", "ns/px", "n", "us", "ns/px"))
for k in list(tb) + [k for k in ts if k not in tb]:
    b, s = tb.get(k, [0, 0.0]), ts.get(k, [0, 0.0])
    r = (b[1] / 786432) / (s[1] / 786432) if s[1] else float("nan")
    print("%-34s %5d %9.1f %9.3f | %5d %9.1f %9.3f | %.2f" % (k[:34], b[0], b[1], b[1] * 1e3 / 786432, s[0], s[1], s[1] * 1e3 / 786432, r))
print("--- big run, in order")
for n, us, g in bigs: print("  %-30s %9.1f %s" % (n[:30], us, g))
print("--- sq12 run, in order")
for n, us, g in sqs: print("  %-30s %9.1f %s" % (n[:30], us, g))
