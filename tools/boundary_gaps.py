#!/usr/bin/env python
"""Where a launch's time ends: per kernel, the dispatch's own duration and the gap to the next dispatch's start.

    rocprofv3 --kernel-trace --output-format csv -d out -- python bench.py --steps 10 --warmup 3 --no-cpu-baseline --no-pmc --no-secondary
    python tools/boundary_gaps.py out/*/*_kernel_trace.csv [--match linear_x3d,attn_x3f] [--json]

A kernel that leaves its output dirty in L2 pays for the write-back either inside its own duration or in the gap before the
next kernel starts; the trace cannot say which, so both are reported and their sum, the PERIOD (start to next start), is
what two store policies are compared by.  Dispatches are ordered by start time per (agent, queue); the gap of a dispatch is
next.start - this.end and is negative when the two overlap.  The last dispatch of a queue has no gap: it counts as a launch
and into the mean duration, but not into the mean gap or period (`closed` = launches that have a successor).

Two tables: by kernel, and by (kernel, next kernel) pair.  Plain Python, no GPU."""
from __future__ import annotations

import argparse
import csv
import json
import re
import sys
from collections import OrderedDict


def short_name(name: str) -> str:
    """'void mi::linear_x3d_kernel<192, true, 1>(mi::ConvGemmDev)' -> 'linear_x3d_kernel<192, true, 1>'"""
    n = name.strip()
    if n.startswith("void "):
        n = n[5:]
    depth = 0
    for i, ch in enumerate(n):                       # cut the parameter list: the first '(' outside template brackets
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            n = n[:i]
            break
    return re.sub(r"\bmi::", "", n)


def read_trace(path: str) -> list:
    """[(queue key, kernel, start ns, end ns)] of a rocprofv3 kernel-trace CSV"""
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            if r.get("Kind", "KERNEL_DISPATCH") != "KERNEL_DISPATCH":
                continue
            rows.append(((r.get("Agent_Id", ""), r.get("Queue_Id", "")), short_name(r["Kernel_Name"]),
                         int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    return rows


class Acc:
    __slots__ = ("launches", "closed", "dur", "gap")

    def __init__(self):
        self.launches = 0; self.closed = 0; self.dur = 0; self.gap = 0

    def row(self) -> dict:
        d = self.dur / self.launches / 1e3
        g = self.gap / self.closed / 1e3 if self.closed else None
        return {"launches": self.launches, "closed": self.closed, "mean_dur_us": d, "mean_gap_us": g,
                "period_us": None if g is None else d + g}


def analyse(rows: list) -> tuple:
    """(by kernel, by (kernel, next kernel)): ordered dicts of name -> row(), sorted by total period, largest first"""
    queues = OrderedDict()
    for q, k, s, e in rows:
        queues.setdefault(q, []).append((s, e, k))
    by_k, by_p = {}, {}
    for lst in queues.values():
        lst.sort(key=lambda t: (t[0], t[1]))
        for i, (s, e, k) in enumerate(lst):
            a = by_k.setdefault(k, Acc())
            a.launches += 1; a.dur += e - s
            if i + 1 < len(lst):
                gap = lst[i + 1][0] - e
                a.closed += 1; a.gap += gap
                b = by_p.setdefault((k, lst[i + 1][2]), Acc())
                b.launches += 1; b.closed += 1; b.dur += e - s; b.gap += gap
    order = lambda d: OrderedDict(sorted(d.items(), key=lambda kv: -(kv[1].dur + kv[1].gap)))
    return (OrderedDict((k, a.row()) for k, a in order(by_k).items()),
            OrderedDict((k, a.row()) for k, a in order(by_p).items()))


def _fmt(v) -> str:
    return "      -" if v is None else f"{v:7.2f}"


def render(by_k, by_p, match=()) -> str:
    keep = lambda name: not match or any(m in name for m in match)
    out = [f"{'launches':>8} {'dur us':>7} {'gap us':>7} {'period':>7}  kernel"]
    for k, r in by_k.items():
        if keep(k):
            out.append(f"{r['launches']:8d} {_fmt(r['mean_dur_us'])} {_fmt(r['mean_gap_us'])} {_fmt(r['period_us'])}  {k}")
    out.append("")
    out.append(f"{'launches':>8} {'dur us':>7} {'gap us':>7} {'period':>7}  kernel -> next kernel")
    for (k, n), r in by_p.items():
        if keep(k):
            out.append(f"{r['launches']:8d} {_fmt(r['mean_dur_us'])} {_fmt(r['mean_gap_us'])} {_fmt(r['period_us'])}  {k} -> {n}")
    return "\n".join(out)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("csv", nargs="+", help="rocprofv3 kernel-trace CSV file(s); several are pooled")
    ap.add_argument("--match", default="", help="comma-separated substrings: only kernels whose short name holds one of them")
    ap.add_argument("--json", action="store_true", help="one JSON object instead of the tables")
    a = ap.parse_args(argv)
    rows = []
    for i, p in enumerate(a.csv):
        rows += [((i,) + q, k, s, e) for q, k, s, e in read_trace(p)]       # files never chain into each other
    by_k, by_p = analyse(rows)
    match = tuple(m for m in a.match.split(",") if m)
    if a.json:
        keep = lambda name: not match or any(m in name for m in match)
        print(json.dumps({"kernels": {k: r for k, r in by_k.items() if keep(k)},
                          "pairs": {f"{k} -> {n}": r for (k, n), r in by_p.items() if keep(k)}}))
    else:
        print(render(by_k, by_p, match))
    return 0


if __name__ == "__main__":
    sys.exit(main())
