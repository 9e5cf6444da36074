#!/usr/bin/env python3
"""The chain between the kernels of consecutive batches, read from one kernel trace.

Input: the per-dispatch CSV (`*_kernel_trace.csv`) of one

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python bench.py --gpus 1 --steps 200 --warmup 20

run, on its own (no counters beside it, the program after `--`).  bench.py keeps two batches in flight
(sann_batch_run_after): per step one descriptor kernel, one unit kernel, one merge kernel and the runtime's blit
kernels for the status copies.  Unit kernels never overlap, so the step is the unit kernel plus the window between
one unit kernel's end and the next one's start; this tool says how long that window is and what stands in it.

For the timed steps (unit launches `--warmup` .. `--warmup + --steps - 1` in start order) it prints median and range,
in microseconds, of
  window        start(unit s) - end(unit s-1)
  desc late     end(desc s) - end(unit s-1): positive = the descriptor kernel of step s is what unit s waited for;
                and the share of steps in which it is positive
  desc          the descriptor kernel's duration
  merge         start and end of merge s relative to end(unit s)
  copy k        start, relative to the start of the unit kernel that started last before it, and duration of the
                k-th blit copy kernel after that unit kernel's start
The i-th descriptor / merge launch in start order belongs to the i-th unit launch: sann_batch_run enqueues one of each.

    python tools/chain_trace.py kernel_trace.csv [--steps 200 --warmup 20] > profiles/rNN_chain_trace_X.txt
"""
import argparse
import csv
import statistics
import sys


def load(path):
    """[(name, start_ns, end_ns)] sorted by start."""
    rows = []
    with open(path, newline="") as f:
        rd = csv.DictReader(f)
        cols = {c.lower(): c for c in rd.fieldnames or []}
        try:
            kn, ks, ke = cols["kernel_name"], cols["start_timestamp"], cols["end_timestamp"]
        except KeyError as e:
            raise SystemExit(f"{path}: not a kernel trace (no column {e}); columns: {rd.fieldnames}")
        for r in rd:
            rows.append((r[kn], int(r[ks]), int(r[ke])))
    rows.sort(key=lambda r: r[1])
    return rows


def classify(name):
    if "unit_fast_kernel" in name:
        return "unit"
    if "desc_query_kernel" in name or "desc_kernel" in name:
        return "desc"
    if "merge_kernel" in name:
        return "merge"
    if "copyBuffer" in name:
        return "copy"
    return None


def chain(rows, warmup, steps):
    """Per timed step, a dict of the figures above in microseconds (None where a kernel is missing)."""
    by = {"unit": [], "desc": [], "merge": [], "copy": []}
    for name, s, e in rows:
        k = classify(name)
        if k:
            by[k].append((s, e))
    units = by["unit"]
    if len(units) < warmup + steps:
        raise SystemExit(f"{len(units)} unit launches in the trace, {warmup + steps} expected (--warmup + --steps)")
    aligned = len(by["desc"]) == len(units) and len(by["merge"]) == len(units)
    # copies by the unit kernel that started last before them (none for the trace's last unit kernel: what follows it
    # is the caller fetching results, not a step)
    copies = [[] for _ in units]
    u = -1
    for s, e in by["copy"]:
        while u + 1 < len(units) and units[u + 1][0] <= s:
            u += 1
        if 0 <= u < len(units) - 1:
            copies[u].append((s, e))
    out = []
    for i in range(max(warmup, 1), warmup + steps):
        us, ue = units[i]
        ps, pe = units[i - 1]
        d = {"unit": (ue - us) / 1e3, "window": (us - pe) / 1e3}
        if aligned:
            ds, de = by["desc"][i]
            ms, me = by["merge"][i]
            d.update(desc=(de - ds) / 1e3, desc_late=(de - pe) / 1e3, desc_start=(ds - pe) / 1e3,
                     merge_start=(ms - ue) / 1e3, merge_end=(me - ue) / 1e3, merge=(me - ms) / 1e3)
        for k, (cs, ce) in enumerate(copies[i]):
            d[f"copy{k}_start"] = (cs - us) / 1e3
            d[f"copy{k}"] = (ce - cs) / 1e3
        out.append(d)
    return out, {k: len(v) for k, v in by.items()}, aligned


def line(label, vals):
    vals = [v for v in vals if v is not None]
    if not vals:
        return f"{label:<44} (none)"
    return (f"{label:<44} median {statistics.median(vals):9.2f}   min {min(vals):9.2f}   max {max(vals):9.2f}"
            f"   mean {statistics.fmean(vals):9.2f}   n {len(vals)}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("csv")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    steps, counts, aligned = chain(load(a.csv), a.warmup, a.steps)
    col = lambda k: [s.get(k) for s in steps]
    print(f"chain of the timed steps (us): {len(steps)} steps; launches in the trace: " +
          ", ".join(f"{k} {n}" for k, n in counts.items()))
    print(line("unit kernel, duration", col("unit")))
    print(line("window: unit(s) start - unit(s-1) end", col("window")))
    print(line("period: unit + window", [s["unit"] + s["window"] for s in steps]))
    if aligned:
        print(line("desc(s) start - unit(s-1) end", col("desc_start")))
        print(line("desc(s) end - unit(s-1) end (+ = late)", col("desc_late")))
        late = [v for v in col("desc_late") if v is not None and v > 0]
        print(f"{'desc late: share of steps':<44} {len(late)} of {len(steps)} = {100.0 * len(late) / len(steps):.1f} %")
        print(line("desc kernel, duration", col("desc")))
        print(line("merge(s) start - unit(s) end", col("merge_start")))
        print(line("merge(s) end - unit(s) end", col("merge_end")))
        print(line("merge kernel, duration", col("merge")))
    else:
        print("descriptor / merge launches do not pair with the unit launches one to one: not attributed")
    n_copy = max((sum(1 for k in s if k.startswith("copy") and k.endswith("_start")) for s in steps), default=0)
    for k in range(n_copy):
        print(line(f"copy {k}: start - unit(s) start", col(f"copy{k}_start")))
        print(line(f"copy {k}: duration", col(f"copy{k}")))
    return 0


if __name__ == "__main__":
    sys.exit(main())
