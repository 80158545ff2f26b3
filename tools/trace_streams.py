#!/usr/bin/env python3
"""Who shares a hardware queue with whom, over the timed steps of a rocprofv3 --kernel-trace run of bench.py.
Usage: trace_streams.py <dir with *_kernel_trace.csv> [STEPS = 20: the region is the last STEPS steps of the run]
Prints, from the Queue_Id and Stream_Id columns of the trace:
  * per hardware queue: streams mapped to it, kernels, busy share of the region;
  * the share of the region in which kernels of two or more FRAMES run at once (a frame = a stream that runs k_trace_closest);
  * every long k_copy_out (the copy to the host): how long it held its queue, and how long the kernels of OTHER streams that ran
    next on that queue had been kept waiting (start minus the end of their stream's previous kernel);
  * the gap in front of k_shade on its own stream (bounces after the first): the wait for the auxiliary stream's event."""
import csv
import glob
import sys

rows = []
for f in glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"].split("(")[0].replace("void ", ""),
                     r.get("Queue_Id", "?"), r.get("Stream_Id", r.get("Queue_Id", "?"))))
rows.sort()
# the region: the last STEPS steps (a step starts with the first bounce's closest-hit kernel, or k_generate), else the second half
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
firsts = [r[0] for r in rows if r[2].startswith("k_trace_closest<FirstBounce") or r[2].startswith("k_generate")]
t_lo = firsts[-steps] if len(firsts) >= steps else rows[len(rows) // 2][0]
rows = [r for r in rows if r[0] >= t_lo]
t_hi = max(r[1] for r in rows)
span = t_hi - t_lo
print(f"{len(rows)} kernels in {span / 1e6:.2f} ms")


def covered(iv):
    """Length of the union of intervals."""
    tot, end = 0, None
    for s, e in sorted(iv):
        if end is None or s > end:
            tot += e - s
            end = e
        elif e > end:
            tot += e - end
            end = e
    return tot


queues = {}
for s, e, n, q, st in rows:
    queues.setdefault(q, []).append((s, e, n, st))
print(f"{len(queues)} hardware queues, {len({r[4] for r in rows})} streams")
for q, ks in sorted(queues.items()):
    streams = sorted({k[3] for k in ks})
    busy = covered([(k[0], k[1]) for k in ks])
    print(f"  queue {q}: {len(ks):6d} kernels, busy {100.0 * busy / span:5.1f} %, kernel time / busy time {sum(k[1] - k[0] for k in ks) / max(busy, 1):4.2f} "
          f"(1.00: one after the other), streams {' '.join(streams)}")

frames = {r[4] for r in rows if r[2].startswith("k_trace_closest")}
ev = []
for s, e, n, q, st in rows:
    if st in frames:
        ev.append((s, 1, st))
        ev.append((e, -1, st))
ev.sort()
live, last, hist = {}, t_lo, {}
for t, d, st in ev:
    k = sum(1 for v in live.values() if v > 0)
    hist[k] = hist.get(k, 0) + (t - last)
    live[st] = live.get(st, 0) + d
    last = t
print(f"{len(frames)} frames (main streams); share of the region with kernels of k frames' main streams running at once:")
for k in sorted(hist):
    print(f"  {k:2d}: {100.0 * hist[k] / span:5.1f} %")
print(f"  two or more: {100.0 * sum(v for k, v in hist.items() if k >= 2) / span:5.1f} %")

prev_end = {}  # stream -> end of its previous kernel
waits = {}
for i, (s, e, n, q, st) in enumerate(rows):
    waits[i] = s - prev_end[st] if st in prev_end else 0
    prev_end[st] = max(e, prev_end.get(st, 0))
copies = [i for i, r in enumerate(rows) if r[2].startswith("k_copy_out") and r[1] - r[0] > 500000]
if copies:
    held = [rows[i][1] - rows[i][0] for i in copies]
    print(f"{len(copies)} copies to the host: held their queue {min(held) / 1e6:.2f} / {sum(held) / len(held) / 1e6:.2f} / {max(held) / 1e6:.2f} ms (min / mean / max)")
    behind = []
    for i in copies:
        s, e, n, q, st = rows[i]
        # kernels of other streams on the same queue that started right behind the copy, and how long their stream had stood still
        b = [(rows[j][2], waits[j]) for j in range(i + 1, len(rows)) if rows[j][3] == q and rows[j][4] != st and e <= rows[j][0] <= e + 50000]
        if b:
            behind.append(max(b, key=lambda x: x[1]))
    if behind:
        w = [x[1] for x in behind]
        names = {}
        for n, _ in behind:
            names[n] = names.get(n, 0) + 1
        print(f"  {len(behind)} of them had another stream's kernel start within 50 us of their end on the same queue; that stream had stood still for "
              f"{sum(w) / len(w) / 1e6:.2f} ms on average (max {max(w) / 1e6:.2f}): {names}")
    else:
        print("  no other stream's kernel started right behind any of them on the same queue")
shade = [waits[i] for i, r in enumerate(rows) if r[2].startswith("k_shade") and "FirstBounce" not in r[2] and waits[i] > 0]
if shade:
    shade.sort()
    print(f"gap in front of k_shade (bounce > 1) on its stream: median {shade[len(shade) // 2] / 1e3:.1f} us, mean {sum(shade) / len(shade) / 1e3:.1f} us, "
          f"90 % {shade[len(shade) * 9 // 10] / 1e3:.1f} us, {len(shade)} launches")
by = {}
for s, e, n, q, st in rows:
    by.setdefault(n, [0, 0])
    by[n][0] += 1
    by[n][1] += e - s
for n, (c, d) in sorted(by.items(), key=lambda kv: -kv[1][1])[:8]:
    print(f"  {n:40s} {c:6d} launches, {d / c / 1e3:9.1f} us average, {d / span:6.2f} x the wall time in sum")
