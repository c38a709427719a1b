#!/usr/bin/env python3
"""The gather map of a join two ways: row numbers as payloads of the row join,
or the index join on the key columns alone.

10M x 200M, Zipf s 1.05, inner join (classes = 1), radix 8+8 Murmur3 and
NoPartitioning. The key columns are generated on the device once; the two
legs alternate --rounds times on one context, each leg rebinding both sides
and then joining --steps times:
  (a) payloads: key columns plus arange payload columns, then join_rows: the
      only route to the map without phj_join_indices. The first join of a
      round packs both sides into tuples (`R.pack`, `S.pack`);
  (b) indices:  the key columns alone, then join_indices.

Reported per leg and algorithm: wall ms per join (host clock around the
synchronous call: every step of every round, the first join of each round
apart because it carries (a)'s packing), the `*.pack`, `*.p1.*`, `rows.count`
and `rows.emit` timers of the last round's first and last join with their
bytes, algorithmic_bytes, and the device bytes held per side: the bound
columns plus the packed tuple copy where there is one (16 B per tuple).

Checked once per algorithm, outside the timing: the counts are equal, and the
(build row, probe row) pairs of (b) equal columns 1 and 2 of (a)'s rows as
multisets (--no-check skips the multiset comparison, not the counts).

One JSON document: --out FILE (default profiles/indices_bench.json)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import partitionedhashjoin_amd as phj

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--scale", type=float, default=1.0, help="shrink both relations (trial runs)")
ap.add_argument("--no-check", action="store_true")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                              "indices_bench.json"))
args = ap.parse_args()

SEED = 20240601
R_, S_ = phj.SIDE_BUILD, phj.SIDE_PROBE
KEEP = ("R.pack", "S.pack", "R.p1.hist", "R.p1.scan", "R.p1.scatter", "S.p1.hist", "S.p1.scan", "S.p1.scatter",
        "rows.count", "rows.emit")
ALGOS = (("radix-8+8-murmur3", phj.radix_params((8, 8), hash=phj.HASH_MURMUR3)), ("no-partitioning", phj.nopart_params()))

nR, nS = max(2, int(10_000_000 * args.scale)), max(2, int(200_000_000 * args.scale))
gen, donor, c = phj.Context(0), phj.Context(0), phj.Context(0)
gen.generate_sequential(R_, nR, 1)
gen.generate_zipf(S_, nS, 1.05, 1, nR, SEED)
gen.to_columns(R_, payloads=False)
gen.to_columns(S_, payloads=False)
rk, sk = gen.columns_ptr(R_)[0], gen.columns_ptr(S_)[0]
donor.upload_columns(R_, np.arange(nR, dtype=np.int64))   # the row numbers (a) has to materialise
donor.upload_columns(S_, np.arange(nS, dtype=np.int64))
ra, sa = donor.columns_ptr(R_)[0], donor.columns_ptr(S_)[0]


def bind(leg):
    c.bind_columns(R_, rk, ra if leg == "payloads" else None, nR, keepalive=(gen, donor))
    c.bind_columns(S_, sk, sa if leg == "payloads" else None, nS, keepalive=(gen, donor))


def join(leg, p):
    return c.join_rows(p, phj.INNER, phj.NO_ROW) if leg == "payloads" else c.join_indices(p, phj.INNER)


def kept(r):
    return {k: {"ms": round(ms, 4), "bytes": int(b)} for k, ms, b in r.timers() if k in KEEP}


def held(leg):
    out = {}
    for tag, side, n in (("R", R_, nR), ("S", S_, nS)):
        info = c.relation_info(side)
        out[tag] = {"relation": n * 8 * (2 if info.has_payloads else 1), "packed_copy": n * 16 * info.packed}
    return out


def pair_codes(b, p):
    return np.sort(np.asarray(b, dtype=np.int64) * nS + np.asarray(p, dtype=np.int64))


doc = {"build": nR, "probe": nS, "skew": 1.05, "classes": phj.INNER, "steps": args.steps, "rounds": args.rounds,
       "scale": args.scale, "algorithms": []}
for name, p in ALGOS:
    legs = {leg: {"first_ms": [], "later_ms": []} for leg in ("payloads", "indices")}
    counts = {}
    for rnd in range(args.rounds):
        for leg in ("payloads", "indices"):
            bind(leg)
            for step in range(args.steps):
                t0 = time.perf_counter()
                r, n = join(leg, p)
                ms = (time.perf_counter() - t0) * 1e3
                legs[leg]["first_ms" if step == 0 else "later_ms"].append(round(ms, 3))
                if step == 0:
                    legs[leg]["first_join"] = kept(r)
            counts[leg] = n.as_dict()
            legs[leg]["last_join"] = kept(r)
            legs[leg]["algorithmic_bytes"] = int(r.algorithmic_bytes)
            legs[leg]["device_bytes_held"] = held(leg)
    entry = {"algorithm": name, "payloads": legs["payloads"], "indices": legs["indices"], "counts": counts["indices"],
             "counts_equal": counts["payloads"] == counts["indices"]}
    for leg in legs:   # per round: the mean over the round's joins, the packing join included
        f, l = legs[leg]["first_ms"], legs[leg]["later_ms"]
        per = (args.steps - 1)
        legs[leg]["round_ms_per_join"] = [round((f[i] + sum(l[i * per:(i + 1) * per])) / args.steps, 3)
                                          for i in range(args.rounds)]
    a, b = legs["payloads"]["round_ms_per_join"], legs["indices"]["round_ms_per_join"]
    entry["indices_over_payloads_per_round"] = [round(y / x, 4) for x, y in zip(a, b)]
    entry["indices_over_payloads_steady"] = (round(float(np.median(legs["indices"]["later_ms"])) /
                                                   float(np.median(legs["payloads"]["later_ms"])), 4)
                                             if args.steps > 1 else None)
    if not args.no_check:   # (b) is the last result in the context; then (a) once more
        print(f"{name}: comparing the pairs ...", flush=True)
        got = pair_codes(*c.joined_indices())
        bind("payloads")
        join("payloads", p)
        rows = c.joined()
        want = pair_codes(rows[:, 1], rows[:, 2])
        del rows
        entry["pairs_equal"] = bool(np.array_equal(got, want))
        del got, want
    doc["algorithms"].append(entry)
    print(json.dumps(entry), flush=True)
    with open(args.out, "w") as f:   # rewritten after every algorithm: a run cut short keeps what it measured
        json.dump(doc, f, indent=1)
        f.write("\n")
    if not entry["counts_equal"] or entry.get("pairs_equal") is False:
        sys.exit(f"{name}: the two routes disagree: {counts}")
