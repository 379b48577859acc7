#!/usr/bin/env python3
"""What the lane-map refresh costs the timed call, from a rocprofv3 kernel trace of the plain
bench run (measurement helper; the trace is taken alone, no counters in the same run).

Usage: python tools/lane_refresh_trace.py <kernel_trace.csv> <steps> [<out.md>]

The timed call is the window from the 2 * steps -th last `k_traverse` launch to the end of the
trace (tools/timed_window.py).  Per step: the first (kick + drift) traversal's duration, whether
a lane refresh ran beside it (k_hilbert_keys / k_lane_keys started inside it or just before), and the gap from
that traversal's end to the next kernel on its stream, which is the second build's first kernel.
Then the refresh's own kernels, and the runtime's fill kernels (hipMemsetAsync) by stream.
"""
import csv
import re
import sys

TRAV = "k_traverse<false"
REFRESH = ("k_hilbert_keys", "k_lane_keys")
LEAD = 100_000  # ns: the refresh is launched just before the traversal it runs beside
REFRESH_ALL = REFRESH + ("radix_sort_onesweep", "k_lane_clear", "k_lane_bases", "k_lane_scatter")


def short(name):
    name = name.replace("void ", "").replace("(anonymous namespace)::", "")
    name = re.sub(r"ROCPRIM_[0-9]+_NS::", "", name)
    return name.split("(")[0][:90]


def stats(v):
    return f"n {len(v)}, avg {sum(v) / len(v):.1f}, min {min(v):.1f}, max {max(v):.1f} us" if v else "none"


def main():
    path, steps = sys.argv[1], int(sys.argv[2])
    ks = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"]),
                 r["Stream_Id"]) for r in csv.DictReader(open(path)))
    trav = [k for k in ks if TRAV in k[2]]
    if len(trav) < 2 * steps:
        sys.exit(f"only {len(trav)} traversal launches in the trace")
    t0 = trav[-2 * steps][0]
    win = [k for k in ks if k[0] >= t0]
    firsts = [k for k in win if TRAV in k[2] and k[2].rstrip().endswith("1, false>")]
    rows, with_r, without_r, gap_r, gap_n = [], [], [], [], []
    for i, (s, e, _, st) in enumerate(firsts):
        refreshed = any(s - LEAD <= k[0] < e and any(r in k[2] for r in REFRESH) for k in win)
        nxt = next((k for k in win if k[3] == st and k[0] >= e), None)
        gap = (nxt[0] - e) / 1e3 if nxt else float("nan")
        dur = (e - s) / 1e3
        (with_r if refreshed else without_r).append(dur)
        if nxt:
            (gap_r if refreshed else gap_n).append(gap)
        rows.append(f"| {i} | {dur:.1f} | {'yes' if refreshed else ''} | {gap:.1f} | "
                    f"{nxt[2][:40] if nxt else ''} |")
    allf = with_r + without_r
    out = [f"# Lane refresh in the timed call ({steps} steps, window {(win[-1][1] - t0) / 1e6:.3f} ms)", "",
           f"first traversal, all steps: {stats(allf)}",
           f"first traversal, steps with a refresh beside it: {stats(with_r)}",
           f"first traversal, steps without: {stats(without_r)}",
           f"gap to the second build's first kernel, refresh steps: {stats(gap_r)}",
           f"gap to the second build's first kernel, other steps: {stats(gap_n)}", ""]
    seconds = [(k[1] - k[0]) / 1e3 for k in win if TRAV in k[2] and k[2].rstrip().endswith("2, false>")]
    out.append(f"second traversal: {stats(seconds)}")
    out.append("")
    out.append("refresh kernels in the window:")
    for name in REFRESH_ALL:
        d = [(k[1] - k[0]) / 1e3 for k in win if name in k[2]]
        if d:
            out.append(f"- `{name}`: {len(d)} launches, total {sum(d):.1f} us, max {max(d):.1f} us")
    fills = {}
    for k in win:
        if "fillBuffer" in k[2]:
            fills.setdefault(k[3], []).append((k[1] - k[0]) / 1e3)
    out.append("")
    out.append("fill kernels (hipMemsetAsync) in the window:")
    for st, d in sorted(fills.items()):
        out.append(f"- stream {st}: {len(d)} launches, total {sum(d):.1f} us, max {max(d):.1f} us")
    out += ["", "| step | first traversal us | refresh beside | gap us | next kernel on the stream |",
            "|---|---|---|---|---|"] + rows
    text = "\n".join(out) + "\n"
    if len(sys.argv) > 3:
        with open(sys.argv[3], "w") as fh:
            fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
