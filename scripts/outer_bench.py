#!/usr/bin/env python3
"""Outer and anti joins (phj_join_rows) measured beside phj_join_inner, on the
workloads of scripts/inner_bench.py:

(a)  C2's relations: Sequential R (10M, unique keys) x Zipf S (200M, s = 1.05).
(b1) Zipf R (s = 1.05 over [1, 1M], 10M rows) x Sequential S (keys 1 .. 1M).
(b2) the same R x Zipf S of the same distribution, sized as inner_bench.py
     sizes it (the largest power of two of probe rows from 2^14 down whose
     pair count stays at or below --max-rows).
NoPartitioning runs (b) on a build side of --np-dup-scale of that size, one
timed step each (inner_bench.py says why).

Per workload and algorithm: join_inner (total, inner.count, inner.emit) and
join_rows for the class sets 1 (inner), 3 (probe outer), 4 (build anti) and
7 (full outer) with rows.count, rows.emit and rows.build_only, and
`mark_over_count` = rows.count of class set 4 / inner.count: what marking the
hit build tuples costs the count pass.

One JSON document: --out FILE (default: stdout only). --merge-inner PARENT
BRANCH stores two inner_bench.py documents (the parent commit's and this
tree's, same box, same session) under "inner_regression" with, per workload,
whether the branch's median total_ms stays within the parent's median plus
the parent's own run-to-run spread (max - min of its total_ms_runs)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import partitionedhashjoin_amd as phj

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--max-rows", type=int, default=1 << 28)
ap.add_argument("--scale", type=float, default=1.0, help="shrink every relation (trial runs)")
ap.add_argument("--np-dup-scale", type=float, default=0.05,
                help="(b), NoPartitioning: build side and key range at this fraction of the radix runs'")
ap.add_argument("--merge-inner", nargs=2, metavar=("PARENT", "BRANCH"))
ap.add_argument("--out")
args = ap.parse_args()

ALGOS = (("radix-8+8-murmur3", phj.radix_params((8, 8), hash=phj.HASH_MURMUR3)),
         ("nopartitioning-xxh3", phj.nopart_params()))
SEED = 20240601
KINDS = (("inner", phj.INNER), ("probe-outer", phj.PROBE_OUTER), ("build-anti", phj.BUILD_ANTI),
         ("full-outer", phj.FULL_OUTER))


def measure(call, steps, warm=True):
    """call() -> (JoinResult, extra dict)."""
    if warm:
        call()   # warm-up (allocations)
    acc, tot = {}, []
    for _ in range(steps):
        r, extra = call()
        tot.append(r.total_ms)
        for k, ms, _ in r.timers():
            acc[k] = acc.get(k, 0.0) + ms
    out = {"rows": int(r.matches), "total_ms": round(float(np.median(tot)), 3),
           "total_ms_runs": [round(t, 3) for t in tot], "algorithmic_bytes": int(r.algorithmic_bytes),
           "kernels_ms": {k: round(v / steps, 4) for k, v in sorted(acc.items())}}
    out.update(extra)
    return out


def inner_regression(parent_path, branch_path):
    with open(parent_path) as f:
        parent = json.load(f)
    with open(branch_path) as f:
        branch = json.load(f)
    verdicts = []
    for a, b in zip(parent["workloads"], branch["workloads"]):
        assert (a["workload"], a["join"]) == (b["workload"], b["join"])
        pa, pb = a["join_inner"], b["join_inner"]
        spread = max(pa["total_ms_runs"]) - min(pa["total_ms_runs"])
        verdicts.append({"workload": a["workload"], "join": a["join"], "parent_total_ms": pa["total_ms"],
                         "parent_spread_ms": round(spread, 3), "branch_total_ms": pb["total_ms"],
                         "within_parent_spread": bool(pb["total_ms"] <= pa["total_ms"] + spread)})
    return {"parent": parent, "branch": branch, "verdicts": verdicts}


def save():
    if args.out:   # rewritten after every workload: a run cut short keeps what it measured
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


def scaled(n):
    return max(1, int(n * args.scale))


doc = {"steps": args.steps, "max_rows": args.max_rows, "scale": args.scale,
       "np_dup_scale": args.np_dup_scale, "workloads": []}
if args.merge_inner:
    doc["inner_regression"] = inner_regression(*args.merge_inner)
    for v in doc["inner_regression"]["verdicts"]:
        print(json.dumps(v), flush=True)
    save()

c = phj.Context(0)


def run(label, name, p, nR, nS, steps, warm):
    def inner():
        return c.join_inner(p), {}

    def rows(classes):
        def call():
            r, n = c.join_rows(p, classes)
            return r, n.as_dict()
        return call

    entry = {"workload": label, "join": name, "build": nR, "probe": nS,
             "join_inner": measure(inner, steps, warm), "join_rows": {}}
    for kind, classes in KINDS:
        entry["join_rows"][kind] = measure(rows(classes), steps, warm)
    k = entry["join_rows"]
    ic = entry["join_inner"]["kernels_ms"].get("inner.count", 0.0)
    entry["mark_over_count"] = round(k["build-anti"]["kernels_ms"]["rows.count"] / ic, 3) if ic else None
    entry["rows_ok"] = bool(k["inner"]["rows"] == k["inner"]["pairs"] == entry["join_inner"]["rows"]
                            and k["full-outer"]["rows"] == k["full-outer"]["pairs"] + k["full-outer"]["probe_only"]
                            + k["full-outer"]["build_only"]
                            and k["build-anti"]["rows"] == k["full-outer"]["build_only"])
    doc["workloads"].append(entry)
    print(json.dumps(entry), flush=True)
    save()


# (a) unique build keys
nR, nS = scaled(10_000_000), scaled(200_000_000)
c.generate_sequential(phj.SIDE_BUILD, nR, 1)
c.generate_zipf(phj.SIDE_PROBE, nS, 1.05, 1, nR, SEED)
for name, p in ALGOS:
    run("a: Sequential R x Zipf S (C2)", name, p, nR, nS, args.steps, True)


# (b) duplicated build side
def probe_sequential():
    c.generate_sequential(phj.SIDE_PROBE, hi, 1)
    return "b1: Zipf R x Sequential S", hi


def probe_zipf():
    nS = 1 << 14
    while nS > 1:
        c.generate_zipf(phj.SIDE_PROBE, nS, 1.05, 1, hi, SEED + 2)
        if c.join_inner_count(ALGOS[0][1]).matches <= args.max_rows:
            break
        nS >>= 1
    return "b2: Zipf R x Zipf S", nS


for (name, p), steps, warm, part in ((ALGOS[0], args.steps, True, 1.0), (ALGOS[1], 1, False, args.np_dup_scale)):
    nR, hi = scaled(10_000_000 * part), scaled(1_000_000 * part)
    c.generate_zipf(phj.SIDE_BUILD, nR, 1.05, 1, hi, SEED + 1)
    for make in (probe_sequential, probe_zipf):
        label, nS = make()
        if not warm:
            c.join_inner_count(p)   # allocates, as inner_bench.py's count call does
        run(label, name, p, nR, nS, steps, warm)
