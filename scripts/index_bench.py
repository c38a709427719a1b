#!/usr/bin/env python3
"""The retained key index (phj_index_build / phj_index_lookup) beside the two
per-call ways to the same answer.

A 10M-row build side (keys 1..10M) and 200M Zipf s 1.05 probe keys (the shape
of C4), XXH3, generated on the device once. The key columns are torch tensors;
the rows column every lookup writes is a torch.int64 tensor. Per layout
(`keys`: a key column, stride 1; `tuples`: the ids of the tuple array, stride
2) and per batch size (1M, 16M, 200M keys):
  index.lookup     the index is built once (its build timed apart); then
                   --reps lookups of successive slices are enqueued back to
                   back on torch's current stream (phj_ctx_set_stream) between
                   two torch events: ms per lookup = event time / lookups. The
                   host's wall clock around the same loop and one synchronise
                   is recorded beside it.
  join_indices     phj_join_indices(classes 3, NoPartitioning) with the slice
                   bound as the probe side: wall ms per synchronous call, and
                   its timers
  member.probe     phj_join_member(probe) the same way (it answers found, not
                   the row)
Both per-call ways rebuild R's tables every call and end in a host round trip.

Checked once, outside the timing, at every batch size: rows equal numpy's
lowest-row answer on a 1M sample and torch's on the whole slice (keys are
1..10M at rows 0..10M-1, so row == key - 1), the found count equals the
member call's.

One JSON document: --out FILE (default profiles/index_bench.json)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch   # (first: torch's runtime must see the card before the library opens it)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import partitionedhashjoin_amd as phj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=200, help="lookups enqueued per measurement at the smallest batch")
ap.add_argument("--calls", type=int, default=5, help="synchronous calls per leg of the per-call ways")
ap.add_argument("--scale", type=float, default=1.0, help="shrink everything (trial runs)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "index_bench.json"))
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("index_bench.py measures on a GPU: none is visible")
SEED = 20240601
R_, S_ = phj.SIDE_BUILD, phj.SIDE_PROBE
dev = torch.device("cuda:0")
torch.cuda.init()
P = phj.nopart_params()

nR, nS = max(2, int(10_000_000 * args.scale)), max(2, int(200_000_000 * args.scale))
BATCHES = [max(1, int(b * args.scale)) for b in (1_000_000, 16_000_000, 200_000_000)]
gen = phj.Context(0)
gen.generate_sequential(R_, nR, 1)
gen.generate_zipf(S_, nS, 1.05, 1, int(nR * 1.2), SEED)   # a sixth of the key range is not in R
rt, st = gen.relation_ptr(R_)[0], gen.relation_ptr(S_)[0]
rk = torch.from_numpy(np.ascontiguousarray(gen.download(R_)[:, 0])).to(dev)
sk_host = np.ascontiguousarray(gen.download(S_)[:, 0])
sk = torch.from_numpy(sk_host).to(dev)
rows = torch.empty(nS, dtype=torch.int64, device=dev)
found = torch.empty(nS, dtype=torch.bool, device=dev)
count = torch.zeros(1, dtype=torch.int64, device=dev)
torch.cuda.synchronize()

ctx = phj.Context(0)
# One stream of torch's for torch's work, the events and the library's kernels.
# Not torch's default stream: its handle is 0, which phj_ctx_set_stream reads as
# "the context's own stream", and a non-blocking stream does not order itself
# against the default one.
stream = torch.cuda.Stream()
torch.cuda.set_stream(stream)
assert stream.cuda_stream != 0
ctx.set_stream(stream.cuda_stream)

doc = {"build": nR, "probe": nS, "skew": 1.05, "hash": "xxh3", "scale": args.scale, "batches": BATCHES,
       "library": os.environ.get("PHJ_LIB") or "libphj_hip.so", "index": {}, "lookup": {}, "per_call": {}, "checks": {}}


def slices(batch, reps):
    """(offset, n) of `reps` successive batches walking through S, wrapping."""
    out, off = [], 0
    for _ in range(reps):
        if off + batch > nS:
            off = 0
        out.append((off, batch))
        off += batch
    return out


ok = True
for layout, stride, base in (("keys", 1, sk.data_ptr()), ("tuples", 2, st)):
    if layout == "keys":
        ctx.bind_columns(R_, rk.data_ptr(), None, nR, keepalive=rk)
    else:
        ctx.bind_device(R_, rt, nR, keepalive=gen)
    builds = []
    for _ in range(3):   # the build, three times: the first grows the workspace
        t0 = time.perf_counter()
        ix = ctx.build_index(P)
        builds.append({"wall_ms": round((time.perf_counter() - t0) * 1e3, 3),
                       "timers": {k: round(ms, 4) for k, ms, _ in ix.result.timers()},
                       "algorithmic_bytes": int(ix.result.algorithmic_bytes)})
        if len(builds) < 3:
            ix.close()
    doc["index"][layout] = {"builds": builds, "info": ix.info().as_dict()}
    for batch in BATCHES:
        reps = max(3, min(args.reps, args.reps * BATCHES[0] // batch * 4))
        plan = slices(batch, reps)
        for off, n in plan[:2]:   # warm-up
            ix.lookup(base + 8 * stride * off, n, rows.data_ptr() + 8 * off, key_stride=stride)
        torch.cuda.synchronize()
        legs = {}
        for name, fptr, cptr in (("rows", None, None), ("rows+found+count", found.data_ptr(), count.data_ptr())):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(stream)
            for off, n in plan:
                ix.lookup(base + 8 * stride * off, n, rows.data_ptr() + 8 * off,
                          None if fptr is None else fptr + off, cptr, key_stride=stride)
            e1.record(stream)
            ctx.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            torch.cuda.synchronize()
            legs[name] = {"lookups": len(plan), "event_ms_per_lookup": round(e0.elapsed_time(e1) / len(plan), 5),
                          "wall_ms_per_lookup": round(wall / len(plan), 5)}
        legs["bytes_per_lookup"] = batch * (8 * stride + 8)
        doc["lookup"][f"{layout}.{batch}"] = legs
        # the check: the first slice again, against numpy and torch
        rows[:batch].fill_(-7)
        count.zero_()
        ix.lookup(base, batch, rows.data_ptr(), found.data_ptr(), count.data_ptr(), key_stride=stride)
        ctx.synchronize()
        torch.cuda.synchronize()
        want = torch.where(sk[:batch] <= nR, sk[:batch] - 1, torch.full_like(sk[:batch], -1))
        m = min(batch, 1_000_000)
        u, first = np.unique(rk[:].cpu().numpy(), return_index=True) if layout == "keys" and batch == BATCHES[0] else (None, None)
        chk = {"rows_equal_torch": bool(torch.equal(rows[:batch], want)),
               "found_equal_torch": bool(torch.equal(found[:batch], want >= 0)),
               "count": int(count.item()), "count_expected": int((want >= 0).sum().item())}
        if u is not None:
            pos = np.minimum(np.searchsorted(u, sk_host[:m]), len(u) - 1)
            chk["rows_equal_numpy_sample"] = bool(np.array_equal(rows[:m].cpu().numpy(),
                                                                 np.where(u[pos] == sk_host[:m], first[pos], -1)))
        ok = ok and chk["rows_equal_torch"] and chk["found_equal_torch"] and chk["count"] == chk["count_expected"] \
            and chk.get("rows_equal_numpy_sample", True)
        doc["checks"][f"{layout}.{batch}"] = chk
    ix.close()
    # the per-call ways on the same slices (synchronous: wall ms per call)
    for batch in BATCHES:
        plan = slices(batch, args.calls + 1)
        for way in ("join_indices", "member.probe"):
            calls, timers = [], {}
            for i, (off, n) in enumerate(plan):
                if layout == "keys":
                    ctx.bind_columns(S_, sk.data_ptr() + 8 * off, None, n, keepalive=sk)
                else:
                    ctx.bind_device(S_, st + 16 * off, n, keepalive=gen)
                t0 = time.perf_counter()
                if way == "join_indices":
                    r, cnt = ctx.join_indices(P, phj.PROBE_OUTER)
                    matched = int(cnt.pairs)
                else:
                    r, cnt, _, _ = ctx.join_member(P, probe=True, probe_mask_ptr=found.data_ptr() + off)
                    matched = int(cnt.probe_matched)
                ms = (time.perf_counter() - t0) * 1e3
                if i == 0:
                    continue   # (the first call grows the workspace)
                calls.append(round(ms, 3))
                for k, tms, _ in r.timers():
                    timers.setdefault(k, []).append(round(tms, 4))
            doc["per_call"][f"{layout}.{batch}.{way}"] = {
                "call_ms": calls, "call_ms_median": round(float(np.median(calls)), 3),
                "timers_median_ms": {k: round(float(np.median(v)), 4) for k, v in timers.items()},
                "matched_last": matched}

doc["summary_ms"] = {}
for layout in ("keys", "tuples"):
    b = doc["index"][layout]["builds"][-1]
    doc["summary_ms"][f"{layout}.index_build_wall"] = b["wall_ms"]
    doc["summary_ms"][f"{layout}.index.build_timer"] = b["timers"].get("index.build")
    for batch in BATCHES:
        doc["summary_ms"][f"{layout}.{batch}"] = {
            "index.lookup(event)": doc["lookup"][f"{layout}.{batch}"]["rows"]["event_ms_per_lookup"],
            "index.lookup+found+count(event)": doc["lookup"][f"{layout}.{batch}"]["rows+found+count"]["event_ms_per_lookup"],
            "join_indices(call)": doc["per_call"][f"{layout}.{batch}.join_indices"]["call_ms_median"],
            "member.probe(call)": doc["per_call"][f"{layout}.{batch}.member.probe"]["call_ms_median"],
            "member.probe(timer)": doc["per_call"][f"{layout}.{batch}.member.probe"]["timers_median_ms"].get("member.probe")}
doc["checks_ok"] = ok
with open(args.out, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")
print(json.dumps(doc["summary_ms"]), flush=True)
print(json.dumps({"checks_ok": ok}), flush=True)
if not ok:
    sys.exit("a row, a found byte or a count is wrong: see " + args.out)
