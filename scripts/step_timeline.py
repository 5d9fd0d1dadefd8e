#!/usr/bin/env python3
"""One replayed step of the benchmark as a kernel timeline, from a rocprofv3 kernel trace:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python bench.py --steps 6 --warmup 2 \\
        --no-cpu-baseline --no-pmc --kernel-steps 0
    python scripts/step_timeline.py DIR [out.txt]

Per kernel of the step with the shortest span (a hipGraph replay; eager steps carry host launch gaps): start offset,
duration, gap to the end of everything before it (negative: it overlaps a kernel of the other stream), queue / stream.  The
last lines give the step's span, the sum of the durations and, per kernel name, launches and summed duration."""
import collections
import csv
import glob
import sys


def main():
    d = sys.argv[1]
    rows = []
    for f in glob.glob(d + "/**/*kernel_trace.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], r.get("Queue_Id", "?"), r.get("Stream_Id", "?")))
    rows.sort()
    starts = [i for i, r in enumerate(rows) if "edge_vectors_fwd" in r[2]]  # the first kernel of a step
    best = None
    for a, b in zip(starts, starts[1:]):
        span = max(r[1] for r in rows[a:b]) - rows[a][0]
        if best is None or span < best[0]:
            best = (span, a, b)
    if best is None:
        sys.exit("no complete step in the trace")
    step = rows[best[1]:best[2]]
    t0 = step[0][0]
    lines, prev_end = [], t0
    per = collections.OrderedDict()
    for s, e, n, q, st in step:
        short = n.replace("void ", "").replace("nqa::", "").replace("(anonymous namespace)::", "").split("(")[0][:70]
        lines.append(f"{(s - t0) / 1e3:9.1f} us  dur {(e - s) / 1e3:7.1f}  gap {(s - prev_end) / 1e3:6.1f}  q{q}/s{st}  {short}")
        prev_end = max(prev_end, e)
        c = per.setdefault(short, [0, 0])
        c[0] += 1
        c[1] += e - s
    lines.append(f"step span {(max(r[1] for r in step) - t0) / 1e3:.1f} us; {len(step)} kernels; sum of durations {sum(e - s for s, e, *_ in step) / 1e3:.1f} us")
    for n, (k, t) in sorted(per.items(), key=lambda x: -x[1][1]):
        lines.append(f"  {t / 1e3:8.1f} us  {k:3d} x  {n}")
    text = "\n".join(lines) + "\n"
    if len(sys.argv) > 2:
        open(sys.argv[2], "w").write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
