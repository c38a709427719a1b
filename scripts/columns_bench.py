#!/usr/bin/env python3
"""The counting join on relations bound as columns beside the same join on tuples.

Per workload (10M x 200M, Murmur3, radix 8+8: C2 = Zipf s 1.05, C5 = s 1.25,
and s 0.01, near uniform) the relations are generated on the device and
phj_join is timed under PHJ_DEFER_TIMERS | PHJ_LEAN_TIMERS, as bench.py times
it: first with the tuples bound, then after to_columns(payloads=False) on both
sides (the key columns alone: the LDS join reads nothing else). Both legs
alternate --rounds times, --steps joins each after --warmup; the counts are
checked against each other.

Reported per leg: ms per join (host clock around the synchronous join: median,
min and max over every timed step), the S.p1.scatter / build / probe timers
with their bytes from the deferred report, R.p1.scatter from one extra join
with every timer on, S's pass in GB/s of its accounted bytes and as a share of
the HBM peak, and relation_info.packed (0: no tuple copy was made).

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
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--scale", type=float, default=1.0, help="shrink every relation (trial runs)")
ap.add_argument("--out")
args = ap.parse_args()

SEED = 20240601
HBM_PEAK_GBS = 8000.0   # MI355X HBM3E peak (bench.py's)
WORKLOADS = (("C2", 1.05), ("C5", 1.25), ("skew-0.01", 0.01))
R_, S_ = phj.SIDE_BUILD, phj.SIDE_PROBE


def scaled(n):
    return max(2, int(n * args.scale))


def timed(c, p):
    """(wall ms of every step, the deferred timers' per-join means and bytes)."""
    for _ in range(args.warmup):
        c.join(p)
    c.timers_report()
    wall = []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        r = c.join(p)
        wall.append((time.perf_counter() - t0) * 1e3)
    rep = c.timers_report().timers()
    return wall, int(r.matches), {k: (ms / args.steps, int(b) // args.steps) for k, ms, b in rep}


def leg_entry(c, walls, timers, plain):
    ms = {k: round(v[0], 4) for k, v in sorted(timers.items())}
    by = {k: v[1] for k, v in sorted(timers.items())}
    full = {k: (t, int(b)) for k, t, b in plain.timers()}
    e = {"ms_per_join": round(float(np.median(walls)), 4), "ms_min": round(min(walls), 4), "ms_max": round(max(walls), 4),
         "round_medians": [round(float(np.median(w)), 4) for w in np.array_split(np.array(walls), args.rounds)],
         "kernels_ms": ms, "kernels_bytes": by,
         "R.p1.scatter": {"ms": round(full["R.p1.scatter"][0], 4), "bytes": full["R.p1.scatter"][1]},
         "algorithmic_bytes": int(plain.algorithmic_bytes),
         "packed": [c.relation_info(R_).packed, c.relation_info(S_).packed]}
    s_ms, s_b = timers["S.p1.scatter"]
    e["S_pass"] = {"ms": round(s_ms, 4), "bytes_per_tuple": s_b / nS, "GBps": round(s_b / (s_ms * 1e-3) / 1e9, 1),
                   "frac_hbm_peak": round(s_b / (s_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
    return e


c = phj.Context(0)
doc = {"steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "scale": args.scale,
       "lib": os.environ.get("PHJ_LIB", "default"), "hbm_peak_GBps": HBM_PEAK_GBS, "workloads": []}
nR, nS = scaled(10_000_000), scaled(200_000_000)
for name, alpha in WORKLOADS:
    plain = phj.radix_params((8, 8), hash=phj.HASH_MURMUR3)
    fast = type(plain).from_buffer_copy(plain)
    fast.flags = plain.flags | phj.DEFER_TIMERS | phj.LEAN_TIMERS
    walls, timers, count, full = {"tuples": [], "columns": []}, {}, {}, {}
    for rnd in range(args.rounds):
        # tuples, then the same relations as key columns: each round regenerates them
        c.generate_sequential(R_, nR, 1)
        c.generate_zipf(S_, nS, alpha, 1, nR, SEED)
        for leg in ("tuples", "columns"):
            if leg == "columns":
                c.to_columns(R_, payloads=False)
                c.to_columns(S_, payloads=False)
            c.prepare(plain)
            w, count[leg], timers[leg] = timed(c, fast)
            walls[leg] += w
            if rnd == args.rounds - 1:
                full[leg] = c.join(plain)
                entry_leg = leg_entry(c, walls[leg], timers[leg], full[leg])
                if leg == "tuples":
                    entry = {"workload": name, "skew": alpha, "build": nR, "probe": nS, "tuples": entry_leg}
                else:
                    entry["columns"] = entry_leg
    entry["matches"] = count["tuples"]
    entry["counts_equal"] = count["tuples"] == count["columns"] == int(full["tuples"].matches) == int(full["columns"].matches)
    t, k = entry["tuples"], entry["columns"]
    entry["columns_over_tuples_ms"] = round(k["ms_per_join"] / t["ms_per_join"], 4)
    entry["columns_over_tuples_S_pass"] = round(k["S_pass"]["ms"] / t["S_pass"]["ms"], 4)
    doc["workloads"].append(entry)
    print(json.dumps(entry), flush=True)
    if args.out:   # rewritten after every workload: a run cut short keeps what it measured
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    if not entry["counts_equal"]:
        sys.exit(f"{name}: the counts differ: {count}")
