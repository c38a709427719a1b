"""Aggregates over the join without its rows (phj_join_aggregate) against a
numpy restatement in uint64 arithmetic, which wraps exactly as the device's
64-bit integers do: from searchsorted over sorted R each probe tuple's n
(equal build keys) and A (the sum of their payloads), from a sorted S each
build tuple's partners and the sum of their payloads. Integer sums modulo
2^64 do not depend on the order of the atomics: every comparison is exact.
Payloads are random over the whole int64 range (so sum_b and sum_ab really
wrap) and unique per side (so a group row identifies its build tuple)."""
import ctypes as C
import functools

import numpy as np
import pytest

import partitionedhashjoin_amd as phj
from hashinv import np_edge_keys, np_geometry, np_home, partition_mates
from oracle import oracle as O
from test_gpu_collisions import MATE_BASE, Crowd, codes, filler
from test_gpu_inner import canon, dup_case, expected_inner, small_cases, with_payloads
from test_gpu_materialize import PARAMS

pytestmark = pytest.mark.gpu

IDS = [p[0] for p in PARAMS]
TWO = [("np", phj.nopart_params()), ("radix-8+8", phj.radix_params((8, 8)))]
M64 = (1 << 64) - 1
U = np.uint64


def full_range(keys, seed):
    """keys with unique payloads over all of int64, INT64_MIN and INT64_MAX among them."""
    keys = np.asarray(keys, dtype=np.int64)
    rng = np.random.default_rng(seed)
    pay = rng.integers(-2**63, 2**63 - 1, len(keys), dtype=np.int64, endpoint=True)
    if len(pay) >= 4:
        pay[[0, 1, 2, 3]] = [-2**63, 2**63 - 1, -2**63 + 1, 2**63 - 2]
    assert len(np.unique(pay)) == len(pay)
    return np.stack([keys, pay], axis=1)


def usum(a):
    return int(np.add.reduce(np.asarray(a, dtype=U), dtype=U)) if len(a) else 0


class Expect:
    """Totals (as integers modulo 2^64) and group rows ((|R|, 4) int64, canonical order)."""

    def __init__(self, R, S):
        self.R, self.S = R, S
        order = np.argsort(R[:, 0], kind="stable")
        rk = R[order, 0]
        ra = np.concatenate([[U(0)], np.cumsum(R[order, 1].view(U), dtype=U)])
        lo, hi = np.searchsorted(rk, S[:, 0], "left"), np.searchsorted(rk, S[:, 0], "right")
        n = (hi - lo).astype(U)
        A = ra[hi] - ra[lo]
        pb = np.ascontiguousarray(S[:, 1]).view(U)
        self.pairs = int(n.sum(dtype=U))
        self.probe_matched = int(np.count_nonzero(n))
        self.sum_a, self.sum_b, self.sum_ab = usum(A), usum(n * pb), usum(A * pb)
        sorder = np.argsort(S[:, 0], kind="stable")
        sk = S[sorder, 0]
        sb = np.concatenate([[U(0)], np.cumsum(S[sorder, 1].view(U), dtype=U)])
        lo, hi = np.searchsorted(sk, R[:, 0], "left"), np.searchsorted(sk, R[:, 0], "right")
        rows = np.stack([R[:, 0], R[:, 1], (hi - lo).astype(np.int64), (sb[hi] - sb[lo]).view(np.int64)], axis=1)
        self.rows = gcanon(rows.reshape(-1, 4))
        self.matched_rows = self.rows[self.rows[:, 2] > 0]
        for a in (self.rows, self.matched_rows):
            a.setflags(write=False)

    def totals(self):
        return (self.pairs, self.probe_matched, self.sum_a, self.sum_b, self.sum_ab)


def gcanon(rows):
    """Group rows ordered by the (unique) build payload."""
    rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1, 4)
    return rows[np.argsort(rows[:, 1], kind="stable")]


def totals_of(t):
    return (t.pairs, t.probe_matched, t.sum_a & M64, t.sum_b & M64, t.sum_ab & M64)


def check(ctx, params, E, upload=True):
    """Totals alone, with groups and with the matched groups; the rows' own sums."""
    if upload:
        ctx.upload(phj.SIDE_BUILD, E.R)
        ctx.upload(phj.SIDE_PROBE, E.S)
    r, t = ctx.join_aggregate(params)
    print("totals", totals_of(t), "expected", E.totals())
    assert totals_of(t) == E.totals() and r.matches == E.pairs
    assert ctx.groups().shape == (0, 4)
    r, t = ctx.join_aggregate(params, groups=True)
    assert totals_of(t) == E.totals() and r.matches == E.pairs
    rows = gcanon(ctx.groups())
    assert rows.shape == E.rows.shape
    assert np.array_equal(rows, E.rows)
    part = rows[:, 2].view(U)
    assert usum(part) == E.pairs and usum(rows[:, 3].view(U)) == E.sum_b
    assert usum(rows[:, 1].view(U) * part) == E.sum_a
    r, t = ctx.join_aggregate(params, groups=True, matched_only=True)
    assert totals_of(t) == E.totals()
    assert np.array_equal(gcanon(ctx.groups()), E.matched_rows)
    return r


@functools.lru_cache(maxsize=None)
def dup_expect():
    R, S = dup_case()[:2]
    return Expect(full_range(R[:, 0], 31), full_range(S[:, 0], 32))


@pytest.mark.parametrize("name,params,ordered", PARAMS, ids=IDS)
def test_agg_duplicates_rounds_and_overflow(ctx, name, params, ordered):
    E = dup_expect()
    _, _, total, _, semi = dup_case()
    assert E.pairs == total and E.probe_matched == semi == O.semijoin_count(E.R, E.S)
    assert 0 < len(E.matched_rows) < len(E.rows)
    r = check(ctx, params, E)
    assert ctx.join_inner_count(params).matches == E.pairs
    names = [n for n, _, _ in r.timers()]
    assert "agg.join" in names and "agg.groups" in names


@functools.lru_cache(maxsize=None)
def hot_probe_expect():
    R, S = O.generate_tables(20_000, 400_000, 1.25, 5, threads=4)
    E = Expect(full_range(R[:, 0], 41), full_range(S[:, 0], 42))
    assert E.pairs == E.probe_matched == len(S)
    assert int(E.rows[:, 2].max()) > 20_000   # one build tuple's partners: many items and workgroups
    return E


@pytest.mark.parametrize("name,params,ordered", PARAMS, ids=IDS)
def test_agg_hot_probe_key_on_unique_build_keys(ctx, name, params, ordered):
    check(ctx, params, hot_probe_expect())


@functools.lru_cache(maxsize=None)
def hot_build_expect():
    R = dup_case()[0]
    rng = np.random.default_rng(23)
    sk = rng.integers(-40_000, 40_000, 20_011)
    sk[[17, 4_100, 4_101, 9_000, 20_010]] = 7
    sk[12_345] = -3
    E = Expect(full_range(R[:, 0], 51), full_range(sk, 52))
    assert E.pairs > 5 * 700 + 300
    return E


@pytest.mark.parametrize("name,params,ordered", PARAMS, ids=IDS)
def test_agg_hot_build_key_few_probes(ctx, name, params, ordered):
    # the wide path: the long bucket compared by the whole wave, A reduced over its lanes
    check(ctx, params, hot_build_expect())


@functools.lru_cache(maxsize=None)
def collision_expect(name):
    """Radix: 600 distinct build keys of one partition and one LDS bucket
    (three rounds of one long bucket of distinct keys), a subset probed.
    NoPartitioning: 70 tuples homed in the table's last bucket, whose run of
    full buckets wraps to bucket 0; a subset probed."""
    params = {p[0]: p[1] for p in PARAMS}[name]
    rng = np.random.default_rng(401)
    if name.startswith("radix"):
        G = partition_mates(params, 650, MATE_BASE)
        rk = np.concatenate([G[:600], np.repeat(G[7], 40), filler(rng, 20_000, 1500, G)])
        rng.shuffle(rk)
        c = Crowd(params, G, rk)
        assert c.rounds >= 3 and len(np.unique(G[:600])) == 600 > 256
        sk = np.concatenate([G[0:600:5], np.repeat(G[7], 3), G[600:], filler(rng, 40_000, 3000, G)])
    else:
        A = np_edge_keys(params, "last_of_table", 60)
        F = np_edge_keys(params, "first_of_table", 10)
        edge = np.concatenate([A, F])
        rk = np.concatenate([A[:40], np.repeat(A[11], 30), F, filler(rng, 20_000, 300, edge)])
        rng.shuffle(rk)
        g = nb, nbr, rbits = np_geometry(len(rk), params.table_ratio)
        assert np.all(np_home(codes(params, A), g) == np.uint64(nb - 1))
        assert np.all(np_home(codes(params, F), g) == np.uint64(0))
        sk = np.concatenate([rk[::2], A[40:], np.repeat(A[11], 5), F[:3], filler(rng, 40_000, 300, edge)])
    rng.shuffle(sk)
    E = Expect(full_range(rk, 61), full_range(sk, 62))
    assert 0 < len(E.matched_rows) < len(E.rows)   # some group rows have no partner
    return E


@pytest.mark.parametrize("name,params,ordered", PARAMS, ids=IDS)
def test_agg_crafted_collisions(ctx, name, params, ordered):
    check(ctx, params, collision_expect(name))


@pytest.mark.parametrize("name,params,ordered", PARAMS, ids=IDS)
def test_agg_empty_and_missing(ctx, name, params, ordered):
    for R, S in small_cases():
        E = Expect(full_range(R[:, 0], 71), full_range(S[:, 0], 72))
        assert E.totals() == (0, 0, 0, 0, 0) and len(E.matched_rows) == 0
        assert np.array_equal(E.rows[:, 2:], np.zeros((len(R), 2), dtype=np.int64))
        check(ctx, params, E)


@pytest.mark.parametrize("name,params", TWO, ids=[p[0] for p in TWO])
def test_agg_poisoned_workspace(name, params):
    # the accumulators, the result words and the compaction counts are all
    # written before they are read, never taken as allocated
    with phj.Context(0) as fresh:
        fresh.debug_poison_alloc(0xFF)
        check(fresh, params, dup_expect())


@pytest.mark.parametrize("name,params", TWO, ids=[p[0] for p in TWO])
def test_agg_independent_of_the_row_buffer(ctx, name, params):
    E = hot_build_expect()
    total, rows = expected_inner(E.R, E.S)
    ctx.upload(phj.SIDE_BUILD, E.R)
    ctx.upload(phj.SIDE_PROBE, E.S)
    assert ctx.join_inner(params).matches == total
    r, t = ctx.join_aggregate(params, groups=True)
    assert totals_of(t) == E.totals()
    assert np.array_equal(canon(ctx.joined()), rows)          # the inner rows are still there
    ctx.join_rows(params, phj.FULL_OUTER)
    assert np.array_equal(gcanon(ctx.groups()), E.rows)       # and the groups after a row join
    r2, t2 = ctx.join_aggregate(params, groups=True)
    assert totals_of(t2) == totals_of(t) and np.array_equal(gcanon(ctx.groups()), E.rows)


@pytest.mark.parametrize("name,params", TWO, ids=[p[0] for p in TWO])
def test_agg_beyond_2_32_pairs(ctx, name, params):
    # 65 600^2 = 4 303 360 000 pairs >= 2^32: no error, every total exact
    n = 65_600
    R, S = full_range(np.full(n, 42), 81), full_range(np.full(n, 42), 82)
    sa = sum(int(x) for x in R[:, 1]) & M64
    sb = sum(int(x) for x in S[:, 1]) & M64
    ctx.upload(phj.SIDE_BUILD, R)
    ctx.upload(phj.SIDE_PROBE, S)
    for groups in (False, True):
        r, t = ctx.join_aggregate(params, groups=groups)
        assert r.matches == t.pairs == n * n >= 1 << 32
        assert totals_of(t) == (n * n, n, (n * sa) & M64, (n * sb) & M64, (sa * sb) & M64)
    rows = gcanon(ctx.groups())
    assert rows.shape == (n, 4) and np.all(rows[:, 2] == n) and np.all(rows[:, 3].view(U) == U(sb))
    assert np.array_equal(rows[:, :2], R[np.argsort(R[:, 1])])


def test_agg_refusals(ctx):
    R, S = small_cases()[2]
    ctx.upload(phj.SIDE_BUILD, R)
    ctx.upload(phj.SIDE_PROBE, S)
    p = phj.radix_params((8, 8))
    for flags in (0x2, 0x4, 0x5, 0x80000001):
        r, t = phj.JoinResult(), phj.JoinTotals()
        rc = ctx._L.phj_join_aggregate(ctx._h, C.byref(p), flags, C.byref(r), C.byref(t))
        assert rc == phj._capi.PHJ_ERR_INVALID, flags
    with phj.Context(devices=[0, 0], flags=phj.CTX_LOCAL) as g:
        with pytest.raises(phj.PhjError, match="single-device") as e:
            g.join_aggregate(p)
        assert e.value.code == phj._capi.PHJ_ERR_STATE
