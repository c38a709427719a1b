#!/usr/bin/env python3
"""Ordinals on the key index (phj_index_build_ex / _encode / _accumulate)
beside what they replace.

A 10M-row build side (keys 1..10M, shuffled, so ordinal != key order) and 200M
probe keys at Zipf s 1.05 and at s 0.01, XXH3, generated on the device once.
Everything runs on one torch stream (phj_ctx_set_stream), between torch events
around enqueued calls, --rounds rounds per leg, the legs of one comparison
interleaved inside each round:

  build        the ordinal build against the plain build (wall ms and timers;
               the difference is `index.ordinals`)
  encode       phj_index_encode (this library) | phj_index_lookup on a plain
               index (this library) | phj_index_lookup on a plain index built
               with the parent commit's library (--parent-lib, loaded beside
               this one), on the same batches: 1M, 16M, 200M at s 1.05 and 200M
               at s 0.01
  accumulate   phj_index_accumulate (counts, and counts + sums) | encode
               followed by torch's index_add_ for counts and for sums
  cache        phj_index_accumulate of this library against other builds of the
               same sources (--acc-libs name=path,...: -DPHJ_IX_ACC_CACHE=0 the
               plain global atomics, =1024 another cache size), at both skews
  torch.unique(return_inverse=True) over the 10M keys and over a 200M batch,
               once each, for orientation

Checked once, outside the timing: codes and groups equal torch's over the whole
batch for every library.

One JSON document: --out FILE (default profiles/ordinal_bench.json)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch   # (first: torch's runtime must see the card before the library opens it)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import partitionedhashjoin_amd as phj
from partitionedhashjoin_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--scale", type=float, default=1.0, help="shrink everything (trial runs)")
ap.add_argument("--parent-lib", default="", help="libphj_hip.so of the parent commit, built beforehand")
ap.add_argument("--acc-libs", default="", help="name=path,... other builds of these sources for the accumulate A/B")
ap.add_argument("--no-unique", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ordinal_bench.json"))
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("ordinal_bench.py measures on a GPU: none is visible")
SEED = 20240601
R_, S_ = phj.SIDE_BUILD, phj.SIDE_PROBE
dev = torch.device("cuda:0")
torch.cuda.init()
P = phj.nopart_params()
vp = C.c_void_p


class OtherLib:
    """A second build of the library in this process, through the C ABI alone:
    one context on the shared stream and one index over the bound key column."""

    def __init__(self, path, stream):
        L = self.L = C.CDLL(path)
        for name, (res, argt) in {
                "phj_ctx_create_device": (C.c_int, [C.c_int, C.POINTER(vp)]),
                "phj_ctx_set_stream": (C.c_int, [vp, vp]),
                "phj_relation_bind_columns": (C.c_int, [vp, C.c_int, vp, vp, C.c_uint64]),
                "phj_index_build": (C.c_int, [vp, C.POINTER(_capi.JoinParams), C.POINTER(vp), C.POINTER(_capi.JoinResult)]),
                "phj_index_build_ex": (C.c_int, [vp, C.POINTER(_capi.JoinParams), C.c_uint32, C.POINTER(vp), C.POINTER(_capi.JoinResult)]),
                "phj_index_lookup": (C.c_int, [vp, vp, vp, C.c_uint32, C.c_uint64, vp, vp, vp]),
                "phj_index_accumulate": (C.c_int, [vp, vp, vp, C.c_uint32, vp, C.c_uint32, C.c_uint64, vp, vp, vp]),
                "phj_ctx_destroy": (None, [vp])}.items():
            f = getattr(L, name, None)
            if f is not None:
                f.restype, f.argtypes = res, argt
        self.c = vp()
        self.ok(L.phj_ctx_create_device(0, C.byref(self.c)))
        self.ok(L.phj_ctx_set_stream(self.c, vp(stream)))
        self.ix = vp()

    @staticmethod
    def ok(rc):
        if rc != 0:
            raise RuntimeError(f"a call into a second library failed: {rc}")

    def build(self, keys, n, ordinals):
        r = _capi.JoinResult()
        self.ok(self.L.phj_relation_bind_columns(self.c, R_, vp(keys), vp(0), n))
        if ordinals:
            self.ok(self.L.phj_index_build_ex(self.c, C.byref(P), 1, C.byref(self.ix), C.byref(r)))
        else:
            self.ok(self.L.phj_index_build(self.c, C.byref(P), C.byref(self.ix), C.byref(r)))

    def lookup(self, keys, n, rows):
        self.ok(self.L.phj_index_lookup(self.c, self.ix, vp(keys), 1, n, vp(rows), None, None))

    def accumulate(self, keys, n, counts, values=None, sums=None):
        self.ok(self.L.phj_index_accumulate(self.c, self.ix, vp(keys), 1, vp(values or 0), 1, n, vp(counts), vp(sums or 0), None))


nR, nS = max(2, int(10_000_000 * args.scale)), max(2, int(200_000_000 * args.scale))
BATCHES = [max(1, int(b * args.scale)) for b in (1_000_000, 16_000_000, 200_000_000)]
gen = phj.Context(0)
skews = {}
for skew in (1.05, 0.01):
    gen.generate_zipf(S_, nS, skew, 1, int(nR * 1.2), SEED)   # a sixth of the key range is not in R
    d = gen.download(S_)
    skews[skew] = (torch.from_numpy(np.ascontiguousarray(d[:, 0])).to(dev), torch.from_numpy(np.ascontiguousarray(d[:, 1])).to(dev))
    del d
gen.close()
rk = (torch.randperm(nR, device=dev, generator=torch.Generator(device=dev).manual_seed(7)) + 1).to(torch.int64)
codes = torch.empty(nS, dtype=torch.int64, device=dev)
counts = torch.zeros(nR, dtype=torch.int64, device=dev)
sums = torch.zeros(nR, dtype=torch.int64, device=dev)
torch.cuda.synchronize()

ctx = phj.Context(0)
stream = torch.cuda.Stream()   # not torch's default stream: handle 0 means "the context's own" to phj_ctx_set_stream
torch.cuda.set_stream(stream)
ctx.set_stream(stream.cuda_stream)
ctx.bind_columns(R_, rk.data_ptr(), None, nR, keepalive=rk)

doc = {"build": nR, "probe": nS, "hash": "xxh3", "scale": args.scale, "rounds": args.rounds, "batches": BATCHES,
       "parent_lib": args.parent_lib, "acc_libs": args.acc_libs, "index": {}, "encode": {}, "accumulate": {}, "cache": {},
       "torch_unique_ms": {}, "checks": {}}
ok = True

# ---- the builds ----
for name, flag in (("plain", False), ("ordinals", True)):
    builds = []
    for _ in range(args.rounds + 1):   # (the first grows the workspace)
        t0 = time.perf_counter()
        ix = ctx.build_index(P, ordinals=flag)
        builds.append({"wall_ms": round((time.perf_counter() - t0) * 1e3, 3), "build_ms": round(ix.result.build_ms, 4),
                       "timers": {k: round(ms, 4) for k, ms, _ in ix.result.timers()},
                       "timer_bytes": {k: int(b) for k, _, b in ix.result.timers()}})
        info = ix.info().as_dict()
        ix.close()
    doc["index"][name] = {"builds": builds[1:], "info": info}
plain = ctx.build_index(P)
ordix = ctx.build_index(P, ordinals=True)
first_ptr, distinct = ordix.first_rows_ptr()
assert distinct == nR
parent = None
if args.parent_lib:
    parent = OtherLib(args.parent_lib, stream.cuda_stream)
    parent.build(rk.data_ptr(), nR, False)
others = {}
for item in filter(None, args.acc_libs.split(",")):
    name, path = item.split("=", 1)
    others[name] = OtherLib(path, stream.cuda_stream)
    others[name].build(rk.data_ptr(), nR, True)
torch.cuda.synchronize()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return round(e0.elapsed_time(e1), 4)


def run_legs(legs, reps):
    """{leg: [ms per call, one per round]}: the legs interleaved inside each round, `reps` enqueued calls per timing."""
    out = {k: [] for k in legs}
    for k, fn in legs.items():   # warm-up
        fn()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for k, fn in legs.items():
            out[k].append(round(timed(lambda: [fn() for _ in range(reps)]) / reps, 5))
    return out


# the expectation from torch: the ordinal of key k is the row of k in rk (all distinct)
ord_of_key = torch.full((int(nR * 1.2) + 2,), -1, dtype=torch.int64, device=dev)
ord_of_key[rk] = torch.arange(nR, device=dev)

cases = [(1.05, b) for b in BATCHES] + [(0.01, BATCHES[-1])]
for skew, batch in cases:
    sk, sv = skews[skew]
    tag = f"s{skew}.{batch}"
    reps = max(1, min(50, BATCHES[-1] // batch))
    kp_, vp_, cp_ = sk.data_ptr(), sv.data_ptr(), codes.data_ptr()
    legs = {"encode": lambda: ordix.encode(kp_, batch, cp_),
            "lookup.plain": lambda: plain.lookup(kp_, batch, cp_),
            "lookup.ordinal_index": lambda: ordix.lookup(kp_, batch, cp_)}
    if parent:
        legs["lookup.plain.parent_lib"] = lambda: parent.lookup(kp_, batch, cp_)
    doc["encode"][tag] = run_legs(legs, reps)
    want = ord_of_key[sk[:batch]]
    hit = want >= 0

    def by_torch(with_sums):
        ordix.encode(kp_, batch, cp_)
        c = codes[:batch]
        m = c >= 0
        counts.index_add_(0, c[m], torch.ones_like(c[m]))
        if with_sums:
            sums.index_add_(0, c[m], sv[:batch][m])

    legs = {"accumulate.counts": lambda: ordix.accumulate(kp_, batch, counts.data_ptr()),
            "accumulate.counts+sums": lambda: ordix.accumulate(kp_, batch, counts.data_ptr(), vp_, sums.data_ptr()),
            "encode+index_add_.counts": lambda: by_torch(False),
            "encode+index_add_.counts+sums": lambda: by_torch(True)}
    doc["accumulate"][tag] = run_legs(legs, max(1, reps // 5))
    if others and batch == BATCHES[-1]:
        legs = {"this.counts+sums": lambda: ordix.accumulate(kp_, batch, counts.data_ptr(), vp_, sums.data_ptr()),
                "this.counts": lambda: ordix.accumulate(kp_, batch, counts.data_ptr())}
        for name, o in others.items():
            legs[name + ".counts+sums"] = lambda o=o: o.accumulate(kp_, batch, counts.data_ptr(), vp_, sums.data_ptr())
            legs[name + ".counts"] = lambda o=o: o.accumulate(kp_, batch, counts.data_ptr())
        doc["cache"][tag] = run_legs(legs, 1)
    # the checks, every library once
    ec = torch.zeros(nR, dtype=torch.int64, device=dev).index_add_(0, want[hit], torch.ones_like(want[hit]))
    es = torch.zeros(nR, dtype=torch.int64, device=dev).index_add_(0, want[hit], sv[:batch][hit])
    chk = {}
    codes[:batch].fill_(-7)
    ordix.encode(kp_, batch, cp_)
    torch.cuda.synchronize()
    chk["codes"] = bool(torch.equal(codes[:batch], want))
    for name, fn in [("rows.ordinal_index", lambda: ordix.lookup(kp_, batch, cp_)), ("rows.plain", lambda: plain.lookup(kp_, batch, cp_))] + \
            ([("rows.parent_lib", lambda: parent.lookup(kp_, batch, cp_))] if parent else []):
        codes[:batch].fill_(-7)
        fn()
        torch.cuda.synchronize()
        chk[name] = bool(torch.equal(codes[:batch], want))   # rk is all distinct: row == ordinal
    for name, acc in [("this", ordix.accumulate)] + [(n, o.accumulate) for n, o in others.items()]:
        counts.zero_()
        sums.zero_()
        acc(kp_, batch, counts.data_ptr(), vp_, sums.data_ptr())
        torch.cuda.synchronize()
        chk["groups." + name] = bool(torch.equal(counts, ec) and torch.equal(sums, es))
    ok = ok and all(chk.values())
    doc["checks"][tag] = chk
    del want, hit, ec, es

if not args.no_unique:
    for name, t in (("build_keys", rk), ("batch_200M_s1.05", skews[1.05][0])):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        u, inv = torch.unique(t, return_inverse=True)
        torch.cuda.synchronize()
        doc["torch_unique_ms"][name] = round((time.perf_counter() - t0) * 1e3, 2)
        del u, inv

doc["checks_ok"] = ok
with open(args.out, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")
med = lambda v: round(float(np.median(v)), 4)
print(json.dumps({k: {tag: {leg: med(v) for leg, v in legs.items()} for tag, legs in doc[k].items()}
                  for k in ("encode", "accumulate", "cache")}), flush=True)
print(json.dumps({"index.ordinals_ms": [b["timers"].get("index.ordinals") for b in doc["index"]["ordinals"]["builds"]],
                  "torch_unique_ms": doc["torch_unique_ms"], "checks_ok": ok}), flush=True)
if not ok:
    sys.exit("a code, a row or a group is wrong: see " + args.out)
