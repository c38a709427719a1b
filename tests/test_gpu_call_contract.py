"""What the C ABI answers to bad calls, and that no call depends on the one before it.

(a) A table of bad calls, each made on every entry point that takes
    phj_join_params: the status code and the message each one gets. The order of
    the argument and state checks at an entry point decides both, and callers
    see them. The expectations (tests/golden/call_contract.json) are what the
    library returned before the entry points shared one call prologue; print
    the table of the library under test with
        python tests/test_gpu_call_contract.py > table.json

(b) One context, the LDS join first, then every entry point that used to reset
    only part of the per-call state: each must give the oracle's answer.
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import partitionedhashjoin_amd as phj
from partitionedhashjoin_amd import _capi
from oracle import oracle as O

SEED = 0x9E3779B97F4A7C15
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "call_contract.json")
NR, NS = 1_000, 5_000


def relations():
    rng = np.random.default_rng(7)
    R = np.stack([np.arange(NR, dtype=np.int64), rng.integers(0, 100, NR, dtype=np.int64)], axis=1)
    S = np.stack([rng.integers(0, 2 * NR, NS, dtype=np.int64), rng.integers(0, 100, NS, dtype=np.int64)], axis=1)
    return R, S


def radix(**kw):
    return phj.radix_params((8, 8), hash=phj.HASH_MURMUR3, seed=SEED, **kw)


def nopart(**kw):
    return phj.nopart_params(hash=phj.HASH_XXH3, seed=SEED, **kw)


def with_fields(p, **fields):
    for k, v in fields.items():
        setattr(p, k, v)
    return p


# ---- the contexts a bad call is made on ----

def ctx_tuples():
    R, S = relations()
    c = phj.Context(0)
    c.upload(phj.SIDE_BUILD, R)
    c.upload(phj.SIDE_PROBE, S)
    return c, NS


def ctx_key_columns():   # both sides a key column alone
    R, S = relations()
    c = phj.Context(0)
    c.upload_columns(phj.SIDE_BUILD, R[:, 0])
    c.upload_columns(phj.SIDE_PROBE, S[:, 0])
    return c, NS


def ctx_no_build():
    c = phj.Context(0)
    c.upload(phj.SIDE_PROBE, relations()[1])
    return c, NS


def ctx_no_probe():
    c = phj.Context(0)
    c.upload(phj.SIDE_BUILD, relations()[0])
    return c, 0


def ctx_two_members():   # two members on device 0 (tests/test_gpu_multirank.py)
    R, S = relations()
    c = phj.Context(devices=[0, 0], flags=phj.CTX_LOCAL)
    c.upload(phj.SIDE_BUILD, R)
    c.upload(phj.SIDE_PROBE, S)
    return c, NS


# ---- the entry points that take phj_join_params ----
# call(L, h, p, a): p = byref(params) or None; a = the call's other arguments

class Args:
    def __init__(self, scratch, n_probe):
        base = scratch.columns_ptr(phj.SIDE_PROBE)[0]
        self.probe_mask, self.build_mask, self.dev_count = base, base + 8192, base + 12288
        self.classes = phj.INNER
        self.agg_flags = 0
        self.sides = phj.MEMBER_PROBE
        self.n_probe = n_probe
        self.segs = (phj.Partitioned * 1)()


def _result():
    return C.byref(phj.JoinResult())


def _index(L, h, p, a, ex):
    ix = C.c_void_p()
    rc = (L.phj_index_build_ex(h, p, 0, C.byref(ix), _result()) if ex else L.phj_index_build(h, p, C.byref(ix), _result()))
    if ix.value:
        L.phj_index_destroy(h, ix)
    return rc


def _partitioned(L, h, p, a, call):
    # both sides partitioned with good params first (whatever that answers), so
    # that a good call has its segments and a bad one is refused for its own reason
    g = radix()
    v = phj.Partitioned()
    L.phj_partition(h, phj.SIDE_PROBE, C.byref(g), C.byref(v))
    v = phj.Partitioned()
    L.phj_partition(h, phj.SIDE_BUILD, C.byref(g), C.byref(v))
    a.segs[0] = v
    return call(a.segs)


def _probe_pass1(L, h, p, a):
    keys = np.zeros(max(1, a.n_probe), dtype=np.int64)
    b1 = np.zeros(2049, dtype=np.uint32)
    nb1, codes = C.c_uint32(), C.c_int()
    return L.phj_probe_pass1(h, p, keys.ctypes.data_as(C.c_void_p), a.n_probe, b1.ctypes.data_as(C.c_void_p),
                             C.byref(nb1), C.byref(codes))


ENTRIES = {
    "phj_join": lambda L, h, p, a: L.phj_join(h, p, _result()),
    "phj_prepare": lambda L, h, p, a: L.phj_prepare(h, p),
    "phj_join_materialize": lambda L, h, p, a: L.phj_join_materialize(h, p, _result()),
    "phj_join_inner_count": lambda L, h, p, a: L.phj_join_inner_count(h, p, _result()),
    "phj_join_inner": lambda L, h, p, a: L.phj_join_inner(h, p, _result()),
    "phj_join_rows_count": lambda L, h, p, a: L.phj_join_rows_count(h, p, a.classes, _result(), C.byref(phj.RowCounts())),
    "phj_join_rows": lambda L, h, p, a: L.phj_join_rows(h, p, a.classes, -1, _result(), C.byref(phj.RowCounts())),
    "phj_join_indices": lambda L, h, p, a: L.phj_join_indices(h, p, a.classes, _result(), C.byref(phj.RowCounts())),
    "phj_join_aggregate": lambda L, h, p, a: L.phj_join_aggregate(h, p, a.agg_flags, _result(), C.byref(phj.JoinTotals())),
    "phj_join_member": lambda L, h, p, a: L.phj_join_member(h, p, a.sides, a.probe_mask, a.build_mask, _result(),
                                                            C.byref(phj.MemberCounts())),
    "phj_index_build": lambda L, h, p, a: _index(L, h, p, a, False),
    "phj_index_build_ex": lambda L, h, p, a: _index(L, h, p, a, True),
    "phj_partition": lambda L, h, p, a: L.phj_partition(h, phj.SIDE_PROBE, p, C.byref(phj.Partitioned())),
    "phj_join_partitioned": lambda L, h, p, a: _partitioned(
        L, h, p, a, lambda segs: L.phj_join_partitioned(h, p, 1, segs, _result())),
    "phj_join_partitioned_async": lambda L, h, p, a: _partitioned(
        L, h, p, a, lambda segs: L.phj_join_partitioned_async(h, p, 1, segs, a.dev_count)),
    "phj_probe_pass1": _probe_pass1,
    "phj_debug_poison_chunk_table": lambda L, h, p, a: L.phj_debug_poison_chunk_table(h, phj.SIDE_PROBE, p, 0),
}
ROWS = ["phj_join_rows_count", "phj_join_rows", "phj_join_indices"]

# name -> (context, params or None, entry points (None: all), changes to the other arguments)
BAD_CALLS = {
    "null params": (ctx_tuples, None, None, {}),
    "unknown algorithm": (ctx_tuples, lambda: with_fields(radix(), algo=7), None, {}),
    "unknown hash, radix": (ctx_tuples, lambda: with_fields(radix(), hash=9), None, {}),
    "unknown hash, no partitioning": (ctx_tuples, lambda: with_fields(nopart(), hash=9), None, {}),
    "table_ratio 0.5": (ctx_tuples, lambda: nopart(table_ratio=0.5), None, {}),
    "classes 0, radix": (ctx_tuples, radix, ROWS, {"classes": 0}),
    "classes 0, no partitioning": (ctx_tuples, nopart, ROWS, {"classes": 0}),
    "classes 0, unknown algorithm": (ctx_tuples, lambda: with_fields(radix(), algo=7), ROWS, {"classes": 0}),
    "aggregate flags MATCHED_ONLY alone": (ctx_tuples, radix, ["phj_join_aggregate"], {"agg_flags": phj.AGG_MATCHED_ONLY}),
    "aggregate flags MATCHED_ONLY alone, unknown algorithm": (
        ctx_tuples, lambda: with_fields(radix(), algo=7), ["phj_join_aggregate"], {"agg_flags": phj.AGG_MATCHED_ONLY}),
    "member sides 0": (ctx_tuples, radix, ["phj_join_member"], {"sides": 0}),
    "member sides 0, unknown algorithm": (ctx_tuples, lambda: with_fields(radix(), algo=7), ["phj_join_member"], {"sides": 0}),
    "member side without its mask": (ctx_tuples, radix, ["phj_join_member"],
                                     {"sides": phj.MEMBER_PROBE | phj.MEMBER_BUILD, "build_mask": None}),
    "key columns alone, radix": (ctx_key_columns, radix, None, {}),
    "key columns alone, no partitioning": (ctx_key_columns, nopart, None, {}),
    "key columns alone, unknown algorithm": (ctx_key_columns, lambda: with_fields(radix(), algo=7), None, {}),
    "unbound build side, radix": (ctx_no_build, radix, None, {}),
    "unbound build side, no partitioning": (ctx_no_build, nopart, None, {}),
    "unbound probe side, radix": (ctx_no_probe, radix, None, {}),
    "unbound probe side, no partitioning": (ctx_no_probe, nopart, None, {}),
    "two members, radix": (ctx_two_members, radix, None, {}),
    "two members, no partitioning": (ctx_two_members, nopart, None, {}),
    "two members, null params": (ctx_two_members, None, None, {}),
}


def answers(name):
    """{entry point: [status, message]} of one bad call (message "" with status 0)."""
    make_ctx, make_params, entries, changes = BAD_CALLS[name]
    L = _capi.load()
    out = {}
    with phj.Context(0) as scratch:
        scratch.upload_columns(phj.SIDE_PROBE, np.zeros(2048, dtype=np.int64))
        c, n_probe = make_ctx()
        try:
            for entry in entries or ENTRIES:
                a = Args(scratch, n_probe)
                for k, v in changes.items():
                    setattr(a, k, v)
                params = make_params() if make_params else None
                rc = ENTRIES[entry](L, c._h, C.byref(params) if params is not None else None, a)
                out[entry] = [rc, L.phj_last_error(c._h).decode() if rc != 0 else ""]
                L.phj_ctx_synchronize(c._h)
        finally:
            c.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(BAD_CALLS))
def test_bad_call_answers(ctx, name):
    with open(GOLDEN) as f:
        expect = json.load(f)[name]
    got = answers(name)
    assert sorted(got) == sorted(expect)
    for entry, (rc, msg) in expect.items():
        print(f"{name} | {entry}: {got[entry]}")
        assert got[entry][0] == rc, (name, entry, got[entry], (rc, msg))
        assert got[entry][1].startswith(msg), (name, entry, got[entry], (rc, msg))


# ---- (b) the per-call state reset ----

@pytest.mark.gpu
@pytest.mark.parametrize("count_pin", ["1", "0"])
def test_no_entry_point_depends_on_the_call_before(ctx, count_pin, monkeypatch):
    monkeypatch.setenv("PHJ_COUNT_PIN", count_pin)
    R, S = O.generate_tables(30_000, 400_003, 1.05, 21, threads=4)
    S[::7, 0] += 30_000   # misses
    expect = O.semijoin_count(R, S)
    lo, hi = 100, 20_000
    in_range = int(np.count_nonzero((S[:, 0] >= lo) & (S[:, 0] <= hi)))
    p = phj.radix_params((8, 8), hash=phj.HASH_MURMUR3, seed=SEED)
    assert phj.join_path(p, len(R), len(S)) == phj.PATH_LDS_JOIN
    _, rb = O.partition(S, 1 << 16, True, O.HASH_MURMUR3, SEED, workers=2)
    with phj.Context(0) as c:
        c.upload(phj.SIDE_BUILD, R)
        c.upload(phj.SIDE_PROBE, S)

        def lds_join():
            assert c.join(p).matches == expect

        def materialize():   # (every build key once: a row per probe tuple with a partner)
            assert c.join_materialize(p).matches == expect

        def partitioned():
            c.partition(phj.SIDE_PROBE, p)
            assert c.join_partitioned(p, [c.partition(phj.SIDE_BUILD, p)]).matches == expect

        def count_in_range():
            assert c.count_in_range(phj.SIDE_PROBE, lo, hi) == in_range

        def probe_pass1():
            _, b1, codes = c.probe_pass1(p)
            nb1 = b1.shape[0] - 1
            assert codes and np.array_equal(b1.astype(np.uint64), rb[::(1 << 16) // nb1])

        for after in (materialize, partitioned, count_in_range, probe_pass1):
            lds_join()
            after()
        lds_join()


if __name__ == "__main__":
    json.dump({name: answers(name) for name in BAD_CALLS}, sys.stdout, indent=1, sort_keys=True)
    print()
