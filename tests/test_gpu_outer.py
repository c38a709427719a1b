"""Outer and anti joins (phj_join_rows_count, phj_join_rows) against a numpy
restatement. A join kind is a set of row classes: the inner join's pair rows
(test_gpu_inner.expected_inner), {id, NULL, payloadB} per probe tuple whose
key no build tuple has, {id, payloadA, NULL} per build tuple whose key no
probe tuple has. The oracle has no outer join, so the expectation is computed
here. Payloads are unique on both sides and NULL_PAYLOAD occurs in neither,
so the whole result is compared as a multiset (canon)."""
import functools

import numpy as np
import pytest

import partitionedhashjoin_amd as phj
from oracle import oracle as O
from test_gpu_inner import R_BASE, S_BASE, canon, expected_inner, with_payloads
from test_gpu_materialize import PARAMS

pytestmark = pytest.mark.gpu

IDS = [p[0] for p in PARAMS]
TWO = [("np", phj.nopart_params(), True), ("radix-8+8", phj.radix_params((8, 8)), False)]
NULL = phj.NULL_PAYLOAD
ALL_CLASSES = range(1, 8)
NONE = np.zeros((0, 2), dtype=np.int64)


class Expect:
    """The three row classes of R, S; rows(classes) in canonical order."""

    def __init__(self, R, S):
        self.R, self.S = R, S
        self.pairs, self.pair_rows = expected_inner(R, S) if len(R) and len(S) else (0, np.zeros((0, 3), np.int64))
        so = S[~np.isin(S[:, 0], R[:, 0])]
        bo = R[~np.isin(R[:, 0], S[:, 0])]
        self.probe_rows = np.stack([so[:, 0], np.full(len(so), NULL), so[:, 1]], axis=1).reshape(-1, 3)
        self.build_rows = np.stack([bo[:, 0], bo[:, 1], np.full(len(bo), NULL)], axis=1).reshape(-1, 3)
        self._canon = {}

    def counts(self, classes):
        p = self.pairs
        s = len(self.probe_rows) if classes & phj.ROWS_PROBE_ONLY else 0
        b = len(self.build_rows) if classes & phj.ROWS_BUILD_ONLY else 0
        return p, s, b, (p if classes & phj.ROWS_PAIRS else 0) + s + b

    def rows(self, classes):
        if classes not in self._canon:
            parts = [a for bit, a in ((phj.ROWS_PAIRS, self.pair_rows), (phj.ROWS_PROBE_ONLY, self.probe_rows),
                                      (phj.ROWS_BUILD_ONLY, self.build_rows)) if classes & bit]
            out = canon(np.concatenate(parts))
            out.setflags(write=False)
            self._canon[classes] = out
        return self._canon[classes]


def check(ctx, params, ordered, E, classes, upload=True):
    """join_rows_count and join_rows of one class set against E."""
    if upload:
        ctx.upload(phj.SIDE_BUILD, E.R)
        ctx.upload(phj.SIDE_PROBE, E.S)
    want = E.counts(classes)
    r, n = ctx.join_rows_count(params, classes)
    assert (n.pairs, n.probe_only, n.build_only, n.rows) == want and r.matches == want[3]
    r, n = ctx.join_rows(params, classes, NULL)
    assert (n.pairs, n.probe_only, n.build_only, n.rows) == want and r.matches == want[3]
    got = ctx.joined()
    assert len(got) == want[3]
    assert np.array_equal(canon(got), E.rows(classes))
    # the probe part: every probe tuple's rows contiguous (as many runs as
    # distinct probe payloads), NoPartitioning in input order; then build-only
    nprobe = want[3] - want[2]
    pb = got[:nprobe, 2]
    assert np.all(pb != NULL)
    assert (1 + int(np.count_nonzero(pb[1:] != pb[:-1])) if nprobe else 0) == len(np.unique(pb))
    if ordered:
        assert np.all(pb[1:] >= pb[:-1])
    assert np.all(got[nprobe:, 2] == NULL)
    return got


@functools.lru_cache(maxsize=None)
def build_keys():
    """test_gpu_inner's duplicates (700 > 256 copies of key 7: several LDS
    rounds, a 100-bucket walk) plus key 11, a 600-copy group nobody asks for."""
    rng = np.random.default_rng(11)
    rk = np.concatenate([np.full(700, 7, dtype=np.int64), np.full(300, -3, dtype=np.int64),
                         np.full(600, 11, dtype=np.int64), rng.integers(-20_000, 20_000, 40_000)])
    rng.shuffle(rk)
    return rk, rng


@functools.lru_cache(maxsize=None)
def rounds_case():
    """9 984 probe copies of key 7 (> 2 x 4096: its partition is joined by
    three items whose flag writes overlap)."""
    rk, rng = build_keys()
    sk = rng.integers(-40_000, 40_000, 60_000)
    sk[sk == 11] = 12
    sk[::6] = 7
    sk[5::601] = -3
    E = Expect(with_payloads(rk, R_BASE), with_payloads(sk, S_BASE))
    assert E.pairs > 0 and len(E.probe_rows) > 0 and len(E.build_rows) > 0
    assert int(np.count_nonzero(sk == 7)) > 2 * 4096 and not np.any(sk == 11)
    return E


@functools.lru_cache(maxsize=None)
def few_probes_case():
    rk = build_keys()[0]
    sk = np.random.default_rng(23).integers(-40_000, 40_000, 20_011)
    sk[sk == 11] = 12
    sk[sk == 7] = 8
    sk[[17, 4_100, 4_101, 9_000, 20_010]] = 7
    sk[12_345] = -3
    E = Expect(with_payloads(rk, R_BASE), with_payloads(sk, S_BASE))
    assert int(np.count_nonzero(sk == 7)) == 5 and int(np.count_nonzero(sk == -3)) == 1
    assert E.pairs > 5 * 700 + 300 and len(E.probe_rows) > 0 and len(E.build_rows) > 600
    return E


@functools.lru_cache(maxsize=None)
def unique_case():
    R, S = O.generate_tables(20_000, 100_000, 1.25, 5, threads=4)
    E = Expect(R, S)
    assert E.pairs == len(S) and len(E.probe_rows) == 0 and len(E.build_rows) > 0
    return E


@functools.lru_cache(maxsize=None)
def small_cases():
    R = with_payloads(np.arange(1, 1001), R_BASE)
    S = with_payloads(np.arange(5000, 9000), S_BASE)
    one = with_payloads([5], R_BASE)
    return [Expect(R, NONE), Expect(NONE, S), Expect(R, S), Expect(NONE, NONE),
            Expect(one, with_payloads([5], S_BASE)), Expect(one, with_payloads([6], S_BASE))]


@pytest.mark.parametrize("classes", ALL_CLASSES)
@pytest.mark.parametrize("name,params,ordered", PARAMS, ids=IDS)
def test_rows_rounds_overflow_several_items(ctx, name, params, ordered, classes):
    check(ctx, params, ordered, rounds_case(), classes)


@pytest.mark.parametrize("name,params,ordered", PARAMS, ids=IDS)
def test_rows_counts_agree_with_existing_joins(ctx, name, params, ordered):
    E = rounds_case()
    ctx.upload(phj.SIDE_BUILD, E.R)
    ctx.upload(phj.SIDE_PROBE, E.S)
    semi = O.semijoin_count(E.R, E.S)
    before = ctx.join(params).matches
    assert before == semi
    _, n = ctx.join_rows_count(params, phj.FULL_OUTER)
    assert n.pairs == ctx.join_inner_count(params).matches
    assert n.probe_only == len(E.S) - semi
    ctx.join_rows(params, phj.FULL_OUTER)
    assert ctx.join(params).matches == before   # the semi-join count is untouched


@pytest.mark.parametrize("classes", [7, 4, 2])
@pytest.mark.parametrize("name,params,ordered", PARAMS, ids=IDS)
def test_rows_hot_build_key_few_probes(ctx, name, params, ordered, classes):
    # all 700 copies of key 7 marked by a single wave-cooperative compare
    check(ctx, params, ordered, few_probes_case(), classes)


@pytest.mark.parametrize("name,params,ordered", PARAMS, ids=IDS)
def test_rows_unique_build_keys(ctx, name, params, ordered):
    E = unique_case()
    outer = check(ctx, params, ordered, E, phj.PROBE_OUTER)
    assert ctx.join_inner(params).matches == len(E.S)
    assert np.array_equal(canon(outer), canon(ctx.joined()))   # every probe tuple matches: the inner join's rows
    anti = check(ctx, params, ordered, E, phj.BUILD_ANTI, upload=False)
    undrawn = E.R[~np.isin(E.R[:, 0], E.S[:, 0])]
    assert np.array_equal(np.sort(anti[:, 1]), np.sort(undrawn[:, 1]))
    r, n = ctx.join_rows(params, phj.PROBE_ANTI)
    assert r.matches == n.rows == 0 and ctx.joined().shape == (0, 3)


@pytest.mark.parametrize("name,params,ordered", PARAMS, ids=IDS)
def test_rows_empty_and_tiny_sides(ctx, name, params, ordered):
    for E in small_cases():
        for classes in ALL_CLASSES:
            got = check(ctx, params, ordered, E, classes)
            if len(E.R) == 0 or len(E.S) == 0:   # no join ran: the other side's rows in input order
                want = [a for bit, a in ((phj.ROWS_PROBE_ONLY, E.probe_rows), (phj.ROWS_BUILD_ONLY, E.build_rows))
                        if classes & bit]
                assert np.array_equal(got, np.concatenate(want).reshape(-1, 3) if want else got[:0])


@pytest.mark.parametrize("name,params,ordered", TWO, ids=[p[0] for p in TWO])
def test_rows_poisoned_workspace(name, params, ordered):
    # hit flags, the probe-only bitmap and the block counts are cleared or
    # written by the library on every call, never read as allocated
    with phj.Context(0) as fresh:
        fresh.debug_poison_alloc(0xFF)
        check(fresh, params, ordered, rounds_case(), phj.FULL_OUTER)


@pytest.mark.parametrize("name,params,ordered", TWO, ids=[p[0] for p in TWO])
def test_rows_range_limit(ctx, name, params, ordered):
    # 65 600^2 = 4 303 360 000 pairs >= 2^32: counted exactly, not materialised
    n = 65_600
    ctx.upload(phj.SIDE_BUILD, with_payloads(np.full(n, 42), R_BASE))
    ctx.upload(phj.SIDE_PROBE, with_payloads(np.full(n, 42), S_BASE))
    r, c = ctx.join_rows_count(params, phj.FULL_OUTER)
    assert (c.pairs, c.probe_only, c.build_only, c.rows) == (n * n, 0, 0, n * n) and r.matches == n * n
    with pytest.raises(phj.PhjError) as e:
        ctx.join_rows(params, phj.FULL_OUTER)
    assert e.value.code == phj._capi.PHJ_ERR_RANGE
    assert ctx.joined().shape == (0, 3)
    r, c = ctx.join_rows(params, phj.ROWS_PROBE_ONLY | phj.ROWS_BUILD_ONLY)   # no pair rows asked: no limit met
    assert (c.pairs, c.probe_only, c.build_only, c.rows) == (n * n, 0, 0, 0)
    assert ctx.joined().shape == (0, 3)
    check(ctx, params, ordered, small_cases()[2], phj.FULL_OUTER)   # a small join afterwards is exact
    check(ctx, params, ordered, few_probes_case(), phj.FULL_OUTER)


@pytest.mark.parametrize("name,params,ordered", PARAMS, ids=IDS)
def test_rows_inner_and_materialize_replace_each_other(ctx, name, params, ordered):
    rng = np.random.default_rng(5)
    R = with_payloads(rng.integers(0, 5000, 15_000), R_BASE)   # ~3 copies of each key, a fifth never asked for
    S = with_payloads(rng.integers(-1000, 4000, 50_001), S_BASE)
    E = Expect(R, S)
    hit = S[np.isin(S[:, 0], R[:, 0])]
    assert len(E.probe_rows) > 0 and len(E.build_rows) > 0
    ctx.upload(phj.SIDE_BUILD, R)
    ctx.upload(phj.SIDE_PROBE, S)
    for _ in range(2):
        check(ctx, params, ordered, E, phj.FULL_OUTER, upload=False)
        assert ctx.join_inner(params).matches == E.pairs
        assert np.array_equal(canon(ctx.joined()), E.pair_rows)
        assert ctx.join_materialize(params).matches == len(hit)
        got = canon(ctx.joined())   # by payload_b: one row per matching probe tuple
        assert np.array_equal(got[:, [0, 2]], hit[np.argsort(hit[:, 1])])


def test_rows_count_leaves_earlier_rows(ctx):
    E = small_cases()[2]
    p = phj.radix_params((8, 8))
    kept = check(ctx, p, False, E, phj.FULL_OUTER)
    ctx.join_rows_count(p, phj.BUILD_ANTI)
    assert np.array_equal(ctx.joined(), kept)


@pytest.mark.parametrize("classes", [0, 8, 9, 1 << 31])
def test_rows_bad_classes_refused(ctx, classes):
    E = small_cases()[2]
    ctx.upload(phj.SIDE_BUILD, E.R)
    ctx.upload(phj.SIDE_PROBE, E.S)
    for call in (lambda p: ctx.join_rows_count(p, classes), lambda p: ctx.join_rows(p, classes)):
        for p in (phj.nopart_params(), phj.radix_params((8, 8))):
            with pytest.raises(phj.PhjError) as e:
                call(p)
            assert e.value.code == phj._capi.PHJ_ERR_INVALID


def test_rows_group_context_refused():
    with phj.Context(devices=[0, 0], flags=phj.CTX_LOCAL) as g:
        for call in (lambda p: g.join_rows_count(p, phj.FULL_OUTER), lambda p: g.join_rows(p, phj.FULL_OUTER)):
            with pytest.raises(phj.PhjError, match="single-device") as e:
                call(phj.radix_params((8, 8)))
            assert e.value.code == phj._capi.PHJ_ERR_STATE
