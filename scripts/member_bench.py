#!/usr/bin/env python3
"""Membership joins (phj_join_member) beside the NoPartitioning count they
are built on, and beside torch.isin.

10M x 200M, Zipf s 1.05 (the shape of C4), XXH3. The relations are generated
on the device once; the key columns are torch tensors and every mask is a
torch.bool tensor whose data_ptr() the call writes. The
legs alternate --rounds times, each leg binding both sides and then running
--steps calls:
  join.nopart      phj_join, NoPartitioning, over tuples: `np.build` and
                   `np.probe` are existing, unchanged code, the yardstick
  probe.tuples     member(probe) over tuples        (sides = 1)
  both.tuples      member(probe | build) over tuples (sides = 3)
  probe.keys       member(probe) over the key columns
  both.keys        member(probe | build) over the key columns
The same script under PHJ_LIB=build/libphj_mstore.so (`make
build/libphj_mstore.so HIPDEFS=-DPHJ_MEMBER_MARK_TEST=0`) measures the build
whose marking probe stores a mark for every hit without looking at it first.
Reported per leg: wall ms of every call (host clock around the synchronous
call; the first call of the run apart, it grows the workspace), and per timer
the ms of every call with its median and bytes; algorithmic_bytes.

Checked once, outside the timing: every mask equals torch.isin's, the counts
equal the masks' sums. torch.isin itself is timed once after a warm-up at a
small slice, or the reason it did not run is recorded.

One JSON document: --out FILE (default profiles/member_bench.json)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch   # (first: torch's runtime must see the card before the library opens it)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import partitionedhashjoin_amd as phj

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--scale", type=float, default=1.0, help="shrink both relations (trial runs)")
ap.add_argument("--no-isin", action="store_true")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                              "member_bench.json"))
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("member_bench.py measures on a GPU: none is visible")
SEED = 20240601
R_, S_ = phj.SIDE_BUILD, phj.SIDE_PROBE
dev = torch.device("cuda:0")
torch.cuda.init()
P = phj.nopart_params()

nR, nS = max(2, int(10_000_000 * args.scale)), max(2, int(200_000_000 * args.scale))
gen = phj.Context(0)
gen.generate_sequential(R_, nR, 1)
gen.generate_zipf(S_, nS, 1.05, 1, nR, SEED)
rt, st = gen.relation_ptr(R_)[0], gen.relation_ptr(S_)[0]
rk = torch.from_numpy(np.ascontiguousarray(gen.download(R_)[:, 0])).to(dev)
sk = torch.from_numpy(np.ascontiguousarray(gen.download(S_)[:, 0])).to(dev)
pmask = torch.empty(nS, dtype=torch.bool, device=dev)
bmask = torch.empty(nR, dtype=torch.bool, device=dev)
torch.cuda.synchronize()

ctx = phj.Context(0)


def bind(c, layout):
    if layout == "tuples":
        c.bind_device(R_, rt, nR, keepalive=gen)
        c.bind_device(S_, st, nS, keepalive=gen)
    else:
        c.bind_columns(R_, rk.data_ptr(), None, nR, keepalive=rk)
        c.bind_columns(S_, sk.data_ptr(), None, nS, keepalive=sk)


def member(c, both):
    r, n, _, _ = c.join_member(P, probe=True, build=both, probe_mask_ptr=pmask.data_ptr(),
                               build_mask_ptr=bmask.data_ptr() if both else None)
    return r, n


LEGS = [("join.nopart", ctx, "tuples", None),
        ("probe.tuples", ctx, "tuples", False), ("both.tuples", ctx, "tuples", True),
        ("probe.keys", ctx, "keys", False), ("both.keys", ctx, "keys", True)]

doc = {"build": nR, "probe": nS, "skew": 1.05, "hash": "xxh3", "steps": args.steps, "rounds": args.rounds,
       "scale": args.scale, "library": os.environ.get("PHJ_LIB") or "libphj_hip.so", "legs": {}, "checks": {}}
legs = {name: {"first_call_ms": None, "call_ms": [], "timers": {}} for name, *_ in LEGS}
for rnd in range(args.rounds):
    for name, c, layout, both in LEGS:
        bind(c, layout)
        L = legs[name]
        for step in range(args.steps):
            t0 = time.perf_counter()
            r = c.join(P) if both is None else member(c, both)[0]
            ms = (time.perf_counter() - t0) * 1e3
            if L["first_call_ms"] is None:
                L["first_call_ms"] = round(ms, 3)
                continue
            L["call_ms"].append(round(ms, 3))
            for k, tms, b in r.timers():
                t = L["timers"].setdefault(k, {"ms": [], "bytes": int(b)})
                t["ms"].append(round(tms, 4))
        L["matches"] = int(r.matches)
        L["algorithmic_bytes"] = int(r.algorithmic_bytes)
for name, L in legs.items():
    L["call_ms_median"] = round(float(np.median(L["call_ms"])), 3)
    for t in L["timers"].values():
        t["median_ms"] = round(float(np.median(t["ms"])), 4)
    doc["legs"][name] = L


def med(leg, timer):
    return legs[leg]["timers"][timer]["median_ms"]


doc["summary_ms"] = {
    "np.probe": med("join.nopart", "np.probe"), "np.build": med("join.nopart", "np.build"),
    "member.probe.tuples": med("probe.tuples", "member.probe"), "member.probe.keys": med("probe.keys", "member.probe"),
    "member.probe.tuples.marking": med("both.tuples", "member.probe"),
    "member.probe.keys.marking": med("both.keys", "member.probe"),
    "member.build.tuples": med("both.tuples", "member.build"), "member.build.keys": med("both.keys", "member.build"),
    "marks_cost.tuples": round(legs["both.tuples"]["call_ms_median"] - legs["probe.tuples"]["call_ms_median"], 3),
    "marks_cost.keys": round(legs["both.keys"]["call_ms_median"] - legs["probe.keys"]["call_ms_median"], 3),
}
print(json.dumps(doc["summary_ms"]), flush=True)

# ---- checks and torch.isin, outside the timing ----
isin = {"ran": False}
want_s = want_r = None
if not args.no_isin:
    try:
        torch.isin(sk[:1_000_000], rk[:100_000])   # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        want_s = torch.isin(sk, rk)
        torch.cuda.synchronize()
        isin = {"ran": True, "isin_probe_in_build_ms": round((time.perf_counter() - t0) * 1e3, 3)}
        t0 = time.perf_counter()
        want_r = torch.isin(rk, sk)
        torch.cuda.synchronize()
        isin["isin_build_in_probe_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    except Exception as e:   # (out of memory at this size: recorded, not fatal)
        isin = {"ran": False, "note": f"torch.isin did not fit or failed: {type(e).__name__}: {str(e)[:200]}"}
doc["torch_isin"] = isin
ok = True
for name, c, layout, both in LEGS[1:]:
    bind(c, layout)
    pmask.fill_(True)
    bmask.fill_(True)
    r, n = member(c, bool(both))
    torch.cuda.synchronize()
    chk = {"probe_matched": int(n.probe_matched), "probe_mask_sum": int(pmask.sum()),
           "matches_equal_join": int(n.probe_matched) == legs["join.nopart"]["matches"]}
    if both:
        chk.update(build_matched=int(n.build_matched), build_mask_sum=int(bmask.sum()))
    if want_s is not None:
        chk["probe_mask_equals_isin"] = bool(torch.equal(pmask, want_s))
        if both and want_r is not None:
            chk["build_mask_equals_isin"] = bool(torch.equal(bmask, want_r))
    good = (chk["probe_matched"] == chk["probe_mask_sum"] and chk["matches_equal_join"] and
            chk.get("build_matched") == chk.get("build_mask_sum") and chk.get("probe_mask_equals_isin", True) and
            chk.get("build_mask_equals_isin", True))
    ok = ok and good
    doc["checks"][name] = chk
doc["checks_ok"] = ok
with open(args.out, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")
print(json.dumps({"checks_ok": ok, "torch_isin": isin}), flush=True)
if not ok:
    sys.exit("a mask or a count is wrong: see " + args.out)
