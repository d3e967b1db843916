#!/usr/bin/env python3
"""Idle gaps of the plan hand-over from a `rocprofv3 --kernel-trace` CSV of `bench.py`.

    python3 tools/trace_gaps.py <..._kernel_trace.csv> [--steps 10] [--step-kernel count_balls_kernel]

A step is what lies between two launches of the sizing pass (`--step-kernel`); the last `--steps` of them
are the timed ones.  Per step, from the begin / end stamps of the dispatches (device copies and fills
appear as `__amd_rocclr_*` kernels), two hand-overs:

  link      from the end of the last link kernel to the begin of the first gather kernel: the host wait
            behind the link phase of a plan with split jobs (`split_count_kernel` .. `split_fill_kernel`)
  classify  from the end of `classify_kernel` to the begin of the first link kernel: the mid-plan read-back

and for each of them, averaged over the steps, in microseconds:

  first_gap   end of the phase's last kernel to the begin of the next kernel on the device
  span        the whole hand-over
  idle        the part of the span in which no kernel ran

plus the mean time of the sizing pass itself.  Prints one JSON line.
"""
import argparse
import csv
import json
import re
import statistics


def column(names, *wanted):
    for w in wanted:
        for n in names:
            if n.lower() == w.lower():
                return n
    raise SystemExit("no column %s in %s" % (wanted, names))


def handover(step, is_from, is_to):
    """(first gap, span, idle) in us between the last `from` dispatch and the first `to` dispatch after it"""
    hits = [r for r in step if is_from(r[2])]
    if not hits:
        return None
    t_end = max(r[1] for r in hits)
    to = [r for r in step if r[0] >= t_end and is_to(r[2])]
    between = [r for r in step if r[0] >= t_end and not is_from(r[2])]
    if not to or not between:
        return None
    t_to = to[0][0]
    busy, cursor = 0, t_end
    for b, e, _ in between:
        if b >= t_to:
            break
        busy += max(0, min(e, t_to) - max(b, cursor))
        cursor = max(cursor, e)
    return (between[0][0] - t_end) / 1e3, (t_to - t_end) / 1e3, (t_to - t_end - busy) / 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--step-kernel", default="count_balls_kernel")
    ap.add_argument("--link-regex", default=r"::link_(?!order)\w*kernel")
    ap.add_argument("--gather-regex", default=r"::gather_\w*kernel")
    args = ap.parse_args()
    with open(args.trace, newline="") as f:
        rd = csv.DictReader(f)
        kn = column(rd.fieldnames, "Kernel_Name")
        kb = column(rd.fieldnames, "Start_Timestamp", "BeginNs")
        ke = column(rd.fieldnames, "End_Timestamp", "EndNs")
        rows = sorted(((int(r[kb]), int(r[ke]), r[kn]) for r in rd))
    link, gather = re.compile(args.link_regex), re.compile(args.gather_regex)
    is_link = lambda n: link.search(n) is not None
    is_gather = lambda n: gather.search(n) is not None
    is_classify = lambda n: "classify_kernel" in n
    starts = [i for i, r in enumerate(rows) if args.step_kernel in r[2]]
    if not starts:
        raise SystemExit("no launch of %s in the trace" % args.step_kernel)
    bounds = starts + [len(rows)]
    steps = [rows[bounds[i]:bounds[i + 1]] for i in range(len(starts))][-args.steps:]
    out = {"steps": len(steps)}
    for key, frm, to in (("link", is_link, is_gather), ("classify", is_classify, is_link)):
        g = [x for x in (handover(s, frm, to) for s in steps) if x]
        if g:
            out[key + "_handover_us"] = {k: round(statistics.mean(x[i] for x in g), 1)
                                         for i, k in enumerate(("first_gap", "span", "idle"))}
            out[key + "_handover_us"]["first_gap_min_max"] = [round(min(x[0] for x in g), 1), round(max(x[0] for x in g), 1)]
    sizing = [(r[1] - r[0]) / 1e3 for r in rows if args.step_kernel in r[2]]
    out[args.step_kernel + "_us"] = {"mean": round(statistics.mean(sizing), 1), "calls": len(sizing)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
