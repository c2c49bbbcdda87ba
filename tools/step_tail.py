"""The serial tail of a scoring step in a rocprofv3 kernel trace: per step, the time from the end of the
last loss launch to the end of the step's last kernel, and from the end of the last walk to the end of the
exact pass's last kernel; medians over the timed steps.
  rocprofv3 --kernel-trace --output-format csv -d <dir> -- python bench.py --steps 7 --warmup 3
  python tools/step_tail.py <dir> [--steps 7]
A step starts at the derived-column launch that follows another step's kernels (a trace without derived
columns: at a gap of more than --gap-us microseconds); the timed steps are the last --steps ones."""
import argparse
import csv
import glob
import os
import re
import statistics


def load(root):
    rows = []
    for f in glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            for r in csv.DictReader(fh):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    return rows


def kind(name):
    """loss / fold / probe / exact (sr_tile_kernel<T, R, mode, gather, ...>), or the kernel's short name"""
    m = re.search(r"sr_tile_kernel<\s*\w+,\s*\d+,\s*(\d+),\s*(true|false)", name)
    if m:
        mode, gather = int(m.group(1)), m.group(2) == "true"
        if mode == 0:
            return "probe" if gather else "loss"
        return {2: "exact", 3: "fold"}.get(mode, "tile")
    for k, v in (("sr_fold_walk", "walk"), ("sr_fold_plan", "plan"), ("sr_jsum_levels", "exact"),
                 ("sr_reduce_partials", "reduce"), ("sr_derived", "derived"), ("sr_fold_compact_scan", "scan"),
                 ("sr_fold_compact", "compact")):
        if k in name:
            return v
    return re.sub(r"\(.*", "", name)[:40]


def split_steps(rows, gap_us):
    has_derived = any(kind(n) == "derived" for _, _, n in rows)
    steps, cur, last_end = [], [], None
    for s, e, n in rows:
        k = kind(n)
        if has_derived:
            new = k == "derived" and cur and cur[-1][2] != "derived"
        else:
            new = last_end is not None and s - last_end > gap_us * 1000
        if new:
            steps.append(cur)
            cur = []
        cur.append((s, e, k))
        last_end = e if last_end is None else max(last_end, e)
    if cur:
        steps.append(cur)
    return [st for st in steps if any(k == "loss" for _, _, k in st)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--gap-us", type=float, default=250.0)
    ap.add_argument("--timeline", type=int, default=-1, help="also print this timed step's kernels: start, end (us), kind")
    a = ap.parse_args()
    rows = load(a.dir)
    if not rows:
        raise SystemExit("no kernel trace rows")
    steps = split_steps(rows, a.gap_us)[-a.steps:]
    tails, exact_tails, spans, chains = [], [], [], []
    print(f"{len(steps)} timed steps (us): span | last loss end -> last kernel end | last walk end -> exact end | "
          f"loss launches, walks | kernels after the last loss end")
    for i, st in enumerate(steps):
        t0 = min(s for s, _, _ in st)
        # (the runtime's fill / copy kernels at a step's end are the next call's first memsets)
        own = [x for x in st if not x[2].startswith("__amd_rocclr")]
        t1 = max(e for _, e, _ in own)
        loss_end = max(e for _, e, k in st if k == "loss")
        walks = [e for _, e, k in st if k == "walk"]
        exact = [e for _, e, k in st if k == "exact"]
        tail = (t1 - loss_end) / 1e3
        etail = (max(exact) - max(walks)) / 1e3 if walks and exact else float("nan")
        after = [k for s, _, k in own if s >= loss_end]
        busy_after = sum(e - max(s, loss_end) for s, e, _ in own if e > loss_end) / 1e3
        tails.append(tail)
        spans.append((t1 - t0) / 1e3)
        chains.append(busy_after)
        if etail == etail:
            exact_tails.append(etail)
        print(f"  step {i}: {spans[-1]:8.1f} | {tail:7.1f} | {etail:7.1f} | {sum(k == 'loss' for _, _, k in st)}, "
              f"{len(walks)} | {' '.join(after)}")
    if 0 <= a.timeline < len(steps):
        st = steps[a.timeline]
        t0 = min(s for s, _, _ in st)
        print(f"step {a.timeline}'s kernels (us from the step's first kernel):")
        for s, e, k in st:
            print(f"  {(s - t0) / 1e3:8.1f} {(e - t0) / 1e3:8.1f}  {k}")
    med = statistics.median
    print(f"median span {med(spans):.1f} us")
    print(f"median tail after the last loss launch {med(tails):.1f} us (kernel time inside it, summed: {med(chains):.1f} us)")
    if exact_tails:
        print(f"median last walk end -> exact pass end {med(exact_tails):.1f} us")
    else:
        print("no exact pass in the timed steps")


if __name__ == "__main__":
    main()
