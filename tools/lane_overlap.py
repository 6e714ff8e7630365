#!/usr/bin/env python3
"""From a rocprofv3 --kernel-trace results.db of a bench.py run: do the other proofs' kernels run WHILE a lane-form commitment launch
does?  Per kernel name (LDE, quotient, everything else that is not the lane hash): how many launches there were, how many of them
STARTED while at least one leaf_hash_lane_kernel was executing, and their time inside / outside such intervals.  A kernel whose stream
shares a hardware queue with a lane launch cannot start before that launch ends (tools/experiments/hw_queue_probe.hip), so it shows up
with few starts inside.  Also: the lane launches themselves (count, grid, average duration) and the share of the run's wall time they cover.
usage: lane_overlap.py <results.db>"""
import sqlite3
import sys


def short(name):
    name = str(name).replace("starkhip::", "")
    cut = name.find("(")
    name = name[:cut] if cut > 0 else name
    return name.split("<")[0][:48]


def main():
    cur = sqlite3.connect(sys.argv[1]).cursor()
    views = [r[0] for r in cur.execute("select name from sqlite_master where type in ('table','view')")]
    src = "kernels" if "kernels" in views else next(v for v in views if "kernel_dispatch" in v)
    cols = [r[1] for r in cur.execute(f"pragma table_info({src})")]
    name_col = "name" if "name" in cols else ("kernel_name" if "kernel_name" in cols else None)
    if name_col is None:
        raise SystemExit(f"no kernel names in {src}: {cols}")
    rows = sorted((s, e, short(n)) for s, e, n in cur.execute(f"select start, end, {name_col} from {src}"))
    lane = [(s, e) for s, e, n in rows if n == "leaf_hash_lane_kernel"]
    if not lane:
        raise SystemExit("no leaf_hash_lane_kernel launch in the trace")
    # the union of the lane launches' intervals
    union = []
    for s, e in lane:
        if union and s <= union[-1][1]:
            union[-1][1] = max(union[-1][1], e)
        else:
            union.append([s, e])
    wall = max(e for _, e, _ in rows) - rows[0][0]
    covered = sum(e - s for s, e in union)
    print(f"leaf_hash_lane_kernel: {len(lane)} launches, average {sum(e - s for s, e in lane) / len(lane) / 1e6:.1f} ms; at least one executing "
          f"{covered / 1e6:.0f} of {wall / 1e6:.0f} ms ({covered / wall:.2f})")

    def inside(s, e):
        t, started = 0, False
        for a, b in union:
            if b <= s:
                continue
            if a >= e:
                break
            t += min(e, b) - max(s, a)
            started = started or a <= s < b
        return t, started

    stats = {}
    for s, e, n in rows:
        if n == "leaf_hash_lane_kernel":
            continue
        t_in, started = inside(s, e)
        st = stats.setdefault(n, [0, 0, 0, 0])
        st[0] += 1
        st[1] += started
        st[2] += t_in
        st[3] += (e - s) - t_in
    print(f"{'kernel':48s} {'launches':>8s} {'started beside a lane launch':>29s} {'ms beside':>10s} {'ms apart':>10s}")
    for n, (cnt, started, t_in, t_out) in sorted(stats.items(), key=lambda kv: -(kv[1][2] + kv[1][3]))[:14]:
        print(f"{n:48s} {cnt:8d} {started:18d} ({started / cnt:4.2f})      {t_in / 1e6:10.1f} {t_out / 1e6:10.1f}")


if __name__ == "__main__":
    main()
