"""Timeline of one steady-state step from a rocprofv3 --kernel-trace CSV: per queue, each kernel's start / end and the gap
to its predecessor on the same queue.  usage: timeline.py trace_kernel_trace.csv [step-from-the-end]"""
import csv, re, sys
from collections import defaultdict

def short(name):
    name = re.sub(r"^void ", "", name)
    name = re.sub(r"\(.*$", "", name)
    m = re.match(r"_Z\d+([a-z0-9_]+?)(P|\d|v|I)", name)
    return m.group(1) if name.startswith("_Z") and m else name

def load(path):
    rows = []
    for r in csv.DictReader(open(path)):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), int(r["Queue_Id"]), short(r["Kernel_Name"])))
    rows.sort()
    return rows

def lane_passes(rows):
    """per queue: the launches from a stem_dw kernel to the next tail7 kernel"""
    byq = defaultdict(list)
    for r in rows:
        byq[r[2]].append(r)
    passes = []
    for q, rs in byq.items():
        cur = None
        for r in rs:
            if r[3].startswith("stem_dw"):
                cur = [r]
            elif cur is not None:
                cur.append(r)
                if r[3].startswith("tail7"):
                    passes.append((q, cur))
                    cur = None
    passes.sort(key=lambda p: p[1][0][0])
    return passes

CHAIN_MEMBERS = None

def main():
    path = sys.argv[1]
    back = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    rows = load(path)
    passes = lane_passes(rows)
    # steps: consecutive lane-passes on different queues that overlap in time
    steps = []
    i = 0
    while i + 1 < len(passes):
        a, b = passes[i], passes[i + 1]
        if a[0] != b[0] and b[1][0][0] < a[1][-1][1]:
            steps.append((a, b)); i += 2
        else:
            i += 1
    print(f"{len(rows)} dispatches, {len(passes)} lane-passes, {len(steps)} two-lane steps; launches per lane-pass: "
          f"{sorted(set(len(p[1]) for p in passes))}")
    step = steps[-back]
    prev = steps[-back - 1]
    t0 = min(l[1][0][0] for l in step)
    prev_end = max(l[1][-1][1] for l in prev)
    print(f"\nstep {len(steps) - back} of {len(steps)} (times in us from the step's first kernel start)")
    print(f"end of the previous step's last kernel -> first kernel of this step: {(t0 - prev_end) / 1e3:.2f} us")
    tot = {}
    for q, ks in step:
        print(f"\n### queue {q}\n\n| # | kernel | start us | end us | dur us | gap to predecessor us |\n|---:|---|---:|---:|---:|---:|")
        gaps = []
        for j, (s, e, _, nm) in enumerate(ks):
            gap = (s - ks[j - 1][1]) / 1e3 if j else float("nan")
            if j: gaps.append(gap)
            print(f"| {j + 1} | `{nm}` | {(s - t0) / 1e3:.2f} | {(e - t0) / 1e3:.2f} | {(e - s) / 1e3:.2f} | {'' if j == 0 else f'{gap:.2f}'} |")
        tot[q] = (ks, gaps)
    print()
    t_end = max(l[1][-1][1] for l in step)
    for q, (ks, gaps) in tot.items():
        kt = sum(e - s for s, e, _, _ in ks) / 1e3
        print(f"queue {q}: {len(ks)} launches, kernel time {kt:.2f} us, first start +{(ks[0][0] - t0) / 1e3:.2f} us, last end "
              f"{(ks[-1][1] - t0) / 1e3:.2f} us ({(t_end - ks[-1][1]) / 1e3:.2f} us before the step's last kernel ends), "
              f"sum of {len(gaps)} gaps {sum(gaps):.2f} us (mean {sum(gaps) / len(gaps):.2f}, max {max(gaps):.2f})")
    print(f"step span (first kernel start -> last kernel end): {(t_end - t0) / 1e3:.2f} us")
    # over all steady-state steps
    spans, gsum = [], []
    for st in steps[2:]:
        spans.append((max(l[1][-1][1] for l in st) - min(l[1][0][0] for l in st)) / 1e3)
        for q, ks in st:
            gsum.append(sum(ks[j][0] - ks[j - 1][1] for j in range(1, len(ks))) / 1e3)
    import statistics as S
    print(f"all steps after the first two: span median {S.median(spans):.2f} us (min {min(spans):.2f}, max {max(spans):.2f}); "
          f"sum of gaps per lane-pass median {S.median(gsum):.2f} us (min {min(gsum):.2f}, max {max(gsum):.2f})")
    # the stretch b7.projse .. b10.projse: seven launches (the last seven in front of tail7), or the one chain14 launch
    def stretch(ks):
        ch = [k for k in ks if k[3].startswith("chain14")]
        return ch if ch else ks[-8:-1]
    print()
    for q, ks in step:
        m = stretch(ks)
        print(f"queue {q}: b7.projse .. b10.projse = {len(m)} launch(es), {sum(e - s for s, e, _, _ in m) / 1e3:.2f} us "
              f"(first start -> last end {(m[-1][1] - m[0][0]) / 1e3:.2f} us)")
    first, second = [], []
    for st in steps[2:]:
        for rank, (q, ks) in enumerate(sorted(st, key=lambda l: l[1][0][0])):
            m = stretch(ks)
            (first if rank == 0 else second).append((m[-1][1] - m[0][0]) / 1e3)
    for nm, v in (("lane that starts first", first), ("lane that starts second", second)):
        print(f"all steps after the first two, {nm}: stretch median {S.median(v):.2f} us (min {min(v):.2f}, max {max(v):.2f})")
    lp = [(ks[-1][1] - ks[0][0]) / 1e3 for st in steps[2:] for q, ks in st]
    print(f"lane-pass (first start -> last end) median {S.median(lp):.2f} us; sum of both lanes' stretches per step median "
          f"{S.median([a + b for a, b in zip(first, second)]):.2f} us")
    return step

if __name__ == "__main__":
    main()
