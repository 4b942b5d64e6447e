#!/usr/bin/env python3
"""How much of a propagate's tail and ordering launches lies under a pass-1 launch, and how long the device idles per horizon step,
from the kernel timestamps of a `rocprofv3 --kernel-trace` run (rocpd results.db) of the all-fp32 step.

    python tools/halves_overlap.py RESULTS.db [--parts 2]

For k_tail, k_order_keys and k_order_rank: the share of their wall time (the union of their intervals) that lies inside the union of the
k_pass1_dyn_blk intervals.  Launches of one stream never overlap, so under the two-part propagate that is the time under
the OTHER half's pass 1; the serial propagate reports 0.  Idle: the gaps between consecutive kernels of the union of ALL intervals that
are shorter than --gap-max microseconds (longer ones are the host between propagates), per horizon step = per k_tail launch / --parts.
Per-launch averages of a --stats summary inflate under overlap (two launches share the device); the unions here do not."""
import argparse
import re
import sqlite3


def union(iv):
    out = []
    for s, e in sorted(iv):
        if out and s <= out[-1][1]:
            out[-1][1] = max(out[-1][1], e)
        else:
            out.append([s, e])
    return out


def inside(iv, cover):
    """length of the intervals iv (a union) that lies inside the union cover"""
    tot, j = 0, 0
    for s, e in iv:
        while j < len(cover) and cover[j][1] <= s:
            j += 1
        i = j
        while i < len(cover) and cover[i][0] < e:
            tot += max(0, min(e, cover[i][1]) - max(s, cover[i][0]))
            i += 1
    return tot


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("db")
    ap.add_argument("--parts", type=int, default=1, help="tail launches per horizon step (2: the two-part propagate)")
    ap.add_argument("--gap-max", type=float, default=300.0, help="longest gap (us) still counted as idle inside a propagate")
    a = ap.parse_args()
    cur = sqlite3.connect(a.db).cursor()
    cols = [r[1] for r in cur.execute("pragma table_info(kernels)")]
    s_col, e_col = ("start", "end") if "start" in cols else ("start_timestamp", "end_timestamp")
    rows = list(cur.execute(f'select name, "{s_col}", "{e_col}" from kernels'))
    by = {}
    for name, s, e in rows:
        m = re.search(r"k_\w+", name)
        by.setdefault(m.group(0) if m else name, []).append((s, e))
    p1 = union(by.get("k_pass1_dyn_blk", []))
    print(f"{len(rows)} kernel launches; k_pass1_dyn_blk: {len(by.get('k_pass1_dyn_blk', []))} launches, union {sum(e - s for s, e in p1) / 1e3:.1f} us")
    for k in ("k_tail", "k_order_keys", "k_order_rank"):
        u = union(by.get(k, []))
        wall = sum(e - s for s, e in u)
        if wall:
            print(f"{k:14s} {len(by[k]):6d} launches  wall {wall / 1e3:10.1f} us  under a pass 1: {inside(u, p1) / 1e3:10.1f} us = {100.0 * inside(u, p1) / wall:5.1f} %")
    allu = union([(s, e) for _, s, e in rows])
    gaps = [allu[i + 1][0] - allu[i][1] for i in range(len(allu) - 1)]
    idle = sum(g for g in gaps if g <= a.gap_max * 1e3)
    steps = max(1, len(by.get("k_tail", [])) // a.parts)
    busy = sum(e - s for s, e in allu)
    print(f"device busy (union of all kernels) {busy / 1e3:.1f} us over {steps} horizon steps = {busy / 1e3 / steps:.2f} us per step; "
          f"idle in gaps <= {a.gap_max:.0f} us: {idle / 1e3:.1f} us = {idle / 1e3 / steps:.2f} us per step")


if __name__ == "__main__":
    main()
