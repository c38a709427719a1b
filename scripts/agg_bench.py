#!/usr/bin/env python3
"""Aggregate join (phj_join_aggregate) measured beside what it replaces.

scripts/inner_bench.py's workloads:
(a)  C2's relations: Sequential R (10M, unique keys) x Zipf S (200M, s = 1.05).
(b1) Zipf R (s = 1.05 over [1, 1M], 10M rows) x Sequential S (keys 1 .. 1M).
(b2) the same R x Zipf S, sized as inner_bench sizes it (pairs <= --max-rows).
     NoPartitioning runs (b) on a build side of --np-dup-scale of that size,
     one timed step, as inner_bench does (its table build is quadratic in the
     copies of one key).

Per workload and algorithm:
  join_inner_count            the count pass the totals pass is compared with;
  join_inner + host reduction the rows written, copied back and summed with
                              numpy (one step: the copy dominates): what a
                              caller does without the aggregate;
  totals / groups / groups_matched   join_aggregate in its three forms, with
                              the per-kernel timers and their bytes; for groups
                              the time added over totals, in all and in the
                              accumulating pass (agg.join), and agg.groups (the
                              clear and the compaction).
The totals are checked against the host reduction of the rows.

--baseline-only runs join_inner_count and join_inner alone, so the script also
runs on a library without the aggregate (PHJ_LIB=an A/B build of the parent).

One JSON document: --out FILE (default: stdout only)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import partitionedhashjoin_amd as phj

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--max-rows", type=int, default=1 << 28)
ap.add_argument("--scale", type=float, default=1.0, help="shrink every relation (trial runs)")
ap.add_argument("--np-dup-scale", type=float, default=0.05)
ap.add_argument("--baseline-only", action="store_true")
ap.add_argument("--out")
args = ap.parse_args()

ALGOS = (("radix-8+8-murmur3", phj.radix_params((8, 8), hash=phj.HASH_MURMUR3)),
         ("nopartitioning-xxh3", phj.nopart_params()))
SEED = 20240601
M64 = (1 << 64) - 1


def stats(call, steps, warm=True):
    """Median, spread and mean per-kernel timers of `steps` calls returning a JoinResult."""
    if warm:
        call()
    tot, acc, nbytes = [], {}, {}
    for _ in range(steps):
        r = call()
        tot.append(r.total_ms)
        for k, ms, by in r.timers():
            acc[k] = acc.get(k, 0.0) + ms
            nbytes[k] = int(by)
    return {"matches": int(r.matches), "total_ms": round(float(np.median(tot)), 3),
            "total_ms_min": round(min(tot), 3), "total_ms_max": round(max(tot), 3),
            "total_ms_runs": [round(t, 3) for t in tot], "algorithmic_bytes": int(r.algorithmic_bytes),
            "kernels_ms": {k: round(v / steps, 4) for k, v in sorted(acc.items())},
            "kernels_bytes": dict(sorted(nbytes.items()))}


def record(entry):
    doc["workloads"].append(entry)
    print(json.dumps(entry), flush=True)
    if args.out:   # rewritten after every workload: a run cut short keeps what it measured
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


def scaled(n):
    return max(1, int(n * args.scale))


def usum(a):
    return int(np.add.reduce(a, dtype=np.uint64))


def host_reduction(p):
    """join_inner, the rows copied back and reduced on the host: (entry, totals)."""
    r = c.join_inner(p)
    t0 = time.perf_counter()
    rows = c.joined()
    t1 = time.perf_counter()
    a, b = rows[:, 1].view(np.uint64), rows[:, 2].view(np.uint64)
    tot = (len(rows), usum(a), usum(b), usum(a * b))
    t2 = time.perf_counter()
    return ({"join_inner_total_ms": round(r.total_ms, 3), "copy_back_ms": round((t1 - t0) * 1e3, 1),
             "numpy_reduce_ms": round((t2 - t1) * 1e3, 1), "rows": len(rows)}, tot)


def run(label, nR, nS, name, p, steps, warm):
    entry = {"workload": label, "join": name, "build": nR, "probe": nS}
    entry["join_inner_count"] = stats(lambda: c.join_inner_count(p), steps, warm)
    red, want = host_reduction(p)
    semi = int(c.join(p).matches)   # probe tuples with a partner
    entry["join_inner_host_reduction"] = red
    if not args.baseline_only:
        forms = (("totals", {}), ("groups", {"groups": True}), ("groups_matched", {"groups": True, "matched_only": True}))
        for form, kw in forms:
            entry[form] = stats(lambda: c.join_aggregate(p, **kw)[0], steps, warm)
            t = c.join_aggregate(p, **kw)[1]
            got = (t.pairs, t.probe_matched, t.sum_a & M64, t.sum_b & M64, t.sum_ab & M64)
            entry[form]["totals_ok"] = bool((got[0],) + got[2:] == want and got[1] == semi)
            if kw:
                entry[form]["group_rows"] = len(c.groups())
        tj, cj = entry["totals"]["kernels_ms"]["agg.join"], entry["join_inner_count"]["kernels_ms"]["inner.count"]
        entry["totals_pass_over_count_pass"] = round(tj / cj, 3)
        entry["totals_over_inner_count_total"] = round(entry["totals"]["total_ms"] / entry["join_inner_count"]["total_ms"], 3)
        entry["totals_over_inner_plus_host"] = round(
            entry["totals"]["total_ms"] / (red["join_inner_total_ms"] + red["copy_back_ms"] + red["numpy_reduce_ms"]), 5)
        g = entry["groups"]
        added = g["kernels_ms"]["agg.join"] - tj
        entry["groups_added_total_ms"] = round(g["total_ms"] - entry["totals"]["total_ms"], 3)
        entry["groups_added_join_ms"] = round(added, 4)
        entry["groups_ms"] = g["kernels_ms"].get("agg.groups")
    record(entry)


c = phj.Context(0)
doc = {"steps": args.steps, "max_rows": args.max_rows, "scale": args.scale, "np_dup_scale": args.np_dup_scale,
       "baseline_only": args.baseline_only, "lib": os.environ.get("PHJ_LIB", "default"), "workloads": []}

# (a) unique build keys
nR, nS = scaled(10_000_000), scaled(200_000_000)
c.generate_sequential(phj.SIDE_BUILD, nR, 1)
c.generate_zipf(phj.SIDE_PROBE, nS, 1.05, 1, nR, SEED)
for name, p in ALGOS:
    run("a: Sequential R x Zipf S (C2)", nR, nS, name, p, args.steps, True)


# (b) duplicated build side
def probe_sequential():
    c.generate_sequential(phj.SIDE_PROBE, hi, 1)
    return "b1: Zipf R x Sequential S", hi


def probe_zipf():
    n = 1 << 14
    while n > 1:
        c.generate_zipf(phj.SIDE_PROBE, n, 1.05, 1, hi, SEED + 2)
        if c.join_inner_count(ALGOS[0][1]).matches <= args.max_rows:
            break
        n >>= 1
    return "b2: Zipf R x Zipf S", n


for (name, p), steps, warm, part in ((ALGOS[0], args.steps, True, 1.0), (ALGOS[1], 1, False, args.np_dup_scale)):
    nR, hi = scaled(10_000_000 * part), scaled(1_000_000 * part)
    c.generate_zipf(phj.SIDE_BUILD, nR, 1.05, 1, hi, SEED + 1)
    for make in (probe_sequential, probe_zipf):
        label, nS = make()
        run(label, nR, nS, name, p, steps, warm)
