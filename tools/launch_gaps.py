#!/usr/bin/env python3
"""Launch gaps of the render kernel's back-to-back trains in a rocprofv3 kernel trace.

usage: launch_gaps.py <dir or *_kernel_trace.csv> [--kernel k_render_fast] [--break-us 50] [--min-launches 10]

Reads the per-dispatch start and end times of the product's render kernel (the instrumented instantiations, STATS = true,
are left out), orders them by start time and cuts them into TRAINS: consecutive dispatches on one queue / stream (the
trace's Stream_Id column where it has one that tells streams apart, else Queue_Id) with no pause longer than --break-us
between the end of one and the start of the next -- a pause that long is the host waiting, not a launch gap.  Per train:
the number of launches, the mean and median kernel duration, the mean and median of start[k+1] - end[k], and the train's
span (first start to last end) divided by its launch count.

A plain `python bench.py` run holds both kinds of train: the preconditioning's 50 launches on the scene's own stream and
the warm-up + timed launches on the caller's stream."""
import argparse
import csv
import glob
import os
import statistics
import sys


def product_kernel(name, stem):
    if stem + "<" not in name:
        return False
    fields = [a.strip() for a in name.split("<", 1)[1].split(">")[0].split(",")]
    return len(fields) < 2 or fields[1] != "true"  # STATS is the second template argument


def read_dispatches(path, stem):
    if os.path.isdir(path):
        files = glob.glob(os.path.join(path, "**", "*_kernel_trace.csv"), recursive=True)
        if not files:
            raise SystemExit(f"launch_gaps.py: no *_kernel_trace.csv below {path}")
        path = max(files, key=os.path.getmtime)
    rows = list(csv.DictReader(open(path)))
    streams = {r.get("Stream_Id") for r in rows} - {None, ""}
    column = "Stream_Id" if len(streams) > 1 else "Queue_Id"
    out = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r[column]) for r in rows if product_kernel(r["Kernel_Name"], stem)]
    return sorted(out), column, path


def trains_of(dispatches, break_ns):
    trains = []
    for d in dispatches:
        if trains and trains[-1][-1][2] == d[2] and d[0] - trains[-1][-1][1] <= break_ns:
            trains[-1].append(d)
        else:
            trains.append([d])
    return trains


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--kernel", default="k_render_fast")
    ap.add_argument("--break-us", type=float, default=50.0)
    ap.add_argument("--min-launches", type=int, default=10)
    args = ap.parse_args()
    dispatches, column, path = read_dispatches(args.trace, args.kernel)
    trains = trains_of(dispatches, args.break_us * 1e3)
    print(f"{os.path.basename(path)}: {len(dispatches)} dispatches of {args.kernel}, trains by {column}, cut at pauses above {args.break_us:g} us")
    short = [t for t in trains if len(t) < args.min_launches]
    if short:
        print(f"{len(short)} train(s) of fewer than {args.min_launches} launches ({sum(len(t) for t in short)} dispatches: single launches "
              f"with a host wait behind them) not listed")
    print(f"{column:>10s} {'launches':>8s} {'kernel us mean':>15s} {'median':>8s} {'gap us mean':>12s} {'median':>8s} {'span/launch us':>15s}")
    for t in trains:
        if len(t) < args.min_launches:
            continue
        dur = [(e - s) / 1e3 for s, e, _ in t]
        gap = [(t[k + 1][0] - t[k][1]) / 1e3 for k in range(len(t) - 1)]
        span = (t[-1][1] - t[0][0]) / 1e3 / len(t)
        print(f"{t[0][2]:>10s} {len(t):8d} {statistics.mean(dur):15.2f} {statistics.median(dur):8.2f} {statistics.mean(gap):12.2f} "
              f"{statistics.median(gap):8.2f} {span:15.2f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
