#!/usr/bin/env python3
"""Inner join (phj_join_inner) measured beside phj_join_materialize.

(a) C2's relations: Sequential R (10M, unique keys) x Zipf S (200M, s = 1.05).
    Both calls must produce the same number of rows; total_ms and the
    per-kernel timers of both, same run, same device. join_materialize is
    untouched by the inner join, so it is the baseline.
(b) A duplicated build side: Zipf R (s = 1.05 over [1, 1M], 10M rows) against
    Sequential S (keys 1 .. 1M: every build tuple pairs exactly once) and
    against Zipf S of the same distribution, sized with join_inner_count: the
    largest power of two of probe rows (from 2^14 down) whose pair count stays
    at or below --max-rows (default 2^28, 6.4 GB of rows; the hard limit is
    2^32 - 1).

    NoPartitioning runs (b) on a build side of a twentieth of that size (see below).

One JSON document: --out FILE (default: stdout only)."""
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
ap.add_argument("--out")
args = ap.parse_args()

ALGOS = (("radix-8+8-murmur3", phj.radix_params((8, 8), hash=phj.HASH_MURMUR3)),
         ("nopartitioning-xxh3", phj.nopart_params()))
SEED = 20240601


def measure(call, p, steps, warm=True):
    if warm:
        call(p)   # warm-up (allocations)
    acc, tot = {}, []
    for _ in range(steps):
        r = call(p)
        tot.append(r.total_ms)
        for k, ms, _ in r.timers():
            acc[k] = acc.get(k, 0.0) + ms
    return {"rows": int(r.matches), "total_ms": round(float(np.median(tot)), 3),
            "total_ms_runs": [round(t, 3) for t in tot], "algorithmic_bytes": int(r.algorithmic_bytes),
            "kernels_ms": {k: round(v / steps, 4) for k, v in sorted(acc.items())}}


def record(entry):
    doc["workloads"].append(entry)
    print(json.dumps(entry), flush=True)
    if args.out:   # rewritten after every workload: a run cut short keeps what it measured
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


def scaled(n):
    return max(1, int(n * args.scale))


c = phj.Context(0)
doc = {"steps": args.steps, "max_rows": args.max_rows, "scale": args.scale,
       "np_dup_scale": args.np_dup_scale, "workloads": []}

# (a) unique build keys
nR, nS = scaled(10_000_000), scaled(200_000_000)
c.generate_sequential(phj.SIDE_BUILD, nR, 1)
c.generate_zipf(phj.SIDE_PROBE, nS, 1.05, 1, nR, SEED)
for name, p in ALGOS:
    mat = measure(c.join_materialize, p, args.steps)
    inner = measure(c.join_inner, p, args.steps)
    rows = c.joined(min(1_000_000, inner["rows"]))
    ok = (inner["rows"] == mat["rows"] == c.join_inner_count(p).matches
          and np.array_equal(rows[:, 1], rows[:, 0] - 1) and len(np.unique(rows[:, 2])) == len(rows))
    record({"workload": "a: Sequential R x Zipf S (C2)", "join": name, "build": nR, "probe": nS,
            "rows_ok": bool(ok), "join_materialize": mat, "join_inner": inner,
            "inner_over_materialize": round(inner["total_ms"] / mat["total_ms"], 3)})

# (b) duplicated build side. The NoPartitioning table build walks every full
# bucket behind a key's home bucket for each copy of the key: quadratic in the
# copies of one key, ~0.9M copies of key 1 at full size (~10^11 bucket visits
# with device atomics). Its runs therefore take the build side at
# --np-dup-scale of the size (default 1/20: 500k rows over [1, 50k]), come
# last, and are one timed step each with no warm-up call (the count call
# before it has allocated).


def run_b(label, nS, name, p, steps, warm):
    count = c.join_inner_count(p)
    inner = measure(c.join_inner, p, steps, warm)
    groups = c.joined(min(2_000_000, inner["rows"]))
    # groups contiguous in the slice: a probe payload never comes back
    pb = groups[:, 2]
    runs = 1 + int(np.count_nonzero(pb[1:] != pb[:-1])) if len(pb) else 0
    ok = inner["rows"] == count.matches and runs == len(np.unique(pb))
    record({"workload": label, "join": name, "build": nR, "probe": nS, "pairs": int(count.matches),
            "rows_ok": bool(ok), "join_inner_count_total_ms": round(count.total_ms, 3),
            "join_inner_count_kernels_ms": {k: round(ms, 4) for k, ms, _ in count.timers()},
            "join_inner": inner})


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
        run_b(label, nS, name, p, steps, warm)
