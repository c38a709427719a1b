"""Inner join with duplicate build keys (phj_join_inner_count, phj_join_inner)
against a numpy restatement: one row {id, payloadA, payloadB} per (build
tuple, probe tuple) pair with equal ids. The oracle has no inner join (the
reference's Get() stops at the first hit), so the expectation is computed
here: R sorted by key, searchsorted per probe tuple, rows by repeat + gather.
Every build and probe payload is unique, so comparing the rows as multisets
proves which build tuple stands in each row."""
import functools

import numpy as np
import pytest

import partitionedhashjoin_amd as phj
from oracle import oracle as O
from test_gpu_materialize import PARAMS

pytestmark = pytest.mark.gpu

IDS = [p[0] for p in PARAMS]
TWO = [("np", phj.nopart_params()), ("radix-8+8", phj.radix_params((8, 8)))]
R_BASE, S_BASE = 1_000_000, 5_000_000   # payload = row index + base: unique over both sides


def with_payloads(keys, base):
    keys = np.asarray(keys, dtype=np.int64)
    return np.stack([keys, np.arange(len(keys), dtype=np.int64) + base], axis=1)


def canon(rows):
    """Rows in a canonical order (payloads are unique: by (payload_b, payload_a))."""
    rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1, 3)
    return rows[np.lexsort((rows[:, 1], rows[:, 2]))]


def expected_inner(R, S):
    """(pair count, rows in canonical order) of R join S on the first column."""
    order = np.argsort(R[:, 0], kind="stable")
    rk = R[order, 0]
    lo = np.searchsorted(rk, S[:, 0], side="left")
    hi = np.searchsorted(rk, S[:, 0], side="right")
    cnt = hi - lo
    total = int(cnt.sum())
    si = np.repeat(np.arange(len(S)), cnt)
    first = np.cumsum(cnt) - cnt
    ri = order[np.repeat(lo, cnt) + (np.arange(total) - np.repeat(first, cnt))]
    rows = np.stack([S[si, 0], R[ri, 1], S[si, 1]], axis=1) if total else np.zeros((0, 3), dtype=np.int64)
    return total, canon(rows)


@functools.lru_cache(maxsize=None)
def dup_case():
    """Duplicates across LDS rounds (700 > 256 copies of one key) and bucket
    overflow (700 > 7 slots: a 100-bucket walk); small natural duplicates."""
    rng = np.random.default_rng(11)
    rk = np.concatenate([np.full(700, 7, dtype=np.int64), np.full(300, -3, dtype=np.int64),
                         rng.integers(-20_000, 20_000, 40_000)])
    rng.shuffle(rk)
    sk = rng.integers(-40_000, 40_000, 300_000)
    sk[::600] = 7
    sk[::601] = -3
    R, S = with_payloads(rk, R_BASE), with_payloads(sk, S_BASE)
    total, rows = expected_inner(R, S)
    for a in (R, S, rows):
        a.setflags(write=False)
    return R, S, total, rows, O.semijoin_count(R, S)


@functools.lru_cache(maxsize=None)
def small_cases():
    """(R, S) with an empty probe side, an empty build side, no key in common."""
    R = with_payloads(np.arange(1, 1001), R_BASE)
    S = with_payloads(np.arange(5000, 9000), S_BASE)
    none = np.zeros((0, 2), dtype=np.int64)
    return [(R, none), (none, S), (R, S)]


def check_dup_case(ctx, params, ordered):
    R, S, total, rows, semi = dup_case()
    ctx.upload(phj.SIDE_BUILD, R)
    ctx.upload(phj.SIDE_PROBE, S)
    assert ctx.join_inner_count(params).matches == total
    assert ctx.join_inner(params).matches == total
    got = ctx.joined()
    assert len(got) == total
    assert np.array_equal(canon(got), rows)
    # all rows of one probe tuple are contiguous: as many runs as distinct probe payloads
    pb = got[:, 2]
    assert 1 + int(np.count_nonzero(pb[1:] != pb[:-1])) == len(np.unique(pb))
    if ordered:   # NoPartitioning: groups in input order
        assert np.all(pb[1:] >= pb[:-1])
    return semi


@pytest.mark.parametrize("name,params,ordered", PARAMS, ids=IDS)
def test_inner_duplicates_rounds_and_overflow(ctx, name, params, ordered):
    semi = check_dup_case(ctx, params, ordered)
    assert ctx.join(params).matches == semi   # the semi-join count is untouched


@pytest.mark.parametrize("name,params,ordered", PARAMS, ids=IDS)
def test_inner_hot_build_key_few_probes(ctx, name, params, ordered):
    # the hot keys' long LDS buckets met by one to five probe tuples among
    # ordinary ones: the radix join compares such a bucket with the whole wave
    # in both passes (with many such probe tuples at once, as above, the count
    # pass goes lane by lane)
    R = dup_case()[0]
    rng = np.random.default_rng(23)
    sk = rng.integers(-40_000, 40_000, 20_011)
    sk[[17, 4_100, 4_101, 9_000, 20_010]] = 7
    sk[12_345] = -3
    S = with_payloads(sk, S_BASE)
    total, rows = expected_inner(R, S)
    assert total > 5 * 700 + 300
    ctx.upload(phj.SIDE_BUILD, R)
    ctx.upload(phj.SIDE_PROBE, S)
    assert ctx.join_inner_count(params).matches == total
    assert ctx.join_inner(params).matches == total
    assert np.array_equal(canon(ctx.joined()), rows)


@pytest.mark.parametrize("name,params,ordered", PARAMS, ids=IDS)
def test_inner_unique_build_keys_equals_materialize(ctx, name, params, ordered):
    R, S = O.generate_tables(20_000, 400_000, 1.25, 5, threads=4)
    ctx.upload(phj.SIDE_BUILD, R)
    ctx.upload(phj.SIDE_PROBE, S)
    assert ctx.join_inner_count(params).matches == len(S)
    assert ctx.join_inner(params).matches == len(S)
    inner = canon(ctx.joined())
    assert ctx.join_materialize(params).matches == len(S)
    assert np.array_equal(inner, canon(ctx.joined()))


@pytest.mark.parametrize("name,params,ordered", PARAMS, ids=IDS)
def test_inner_empty_and_missing(ctx, name, params, ordered):
    for R, S in small_cases():
        ctx.upload(phj.SIDE_BUILD, R)
        ctx.upload(phj.SIDE_PROBE, S)
        assert ctx.join_inner_count(params).matches == 0
        assert ctx.join_inner(params).matches == 0
        assert ctx.joined().shape == (0, 3)


@pytest.mark.parametrize("name,params,ordered", PARAMS, ids=IDS)
def test_inner_and_materialize_replace_each_other(ctx, name, params, ordered):
    rng = np.random.default_rng(5)
    R = with_payloads(rng.integers(0, 3000, 9000), R_BASE)     # ~3 copies of each key
    S = with_payloads(rng.integers(-1000, 4000, 50_001), S_BASE)
    total, rows = expected_inner(R, S)
    hit = S[np.isin(S[:, 0], R[:, 0])]
    ctx.upload(phj.SIDE_BUILD, R)
    ctx.upload(phj.SIDE_PROBE, S)
    for _ in range(2):
        assert ctx.join_inner(params).matches == total
        assert np.array_equal(canon(ctx.joined()), rows)
        assert ctx.join_materialize(params).matches == len(hit)
        got = canon(ctx.joined())   # by payload_b: one row per matching probe tuple
        assert np.array_equal(got[:, [0, 2]], hit[np.argsort(hit[:, 1])])
        assert np.all(R[got[:, 1] - R_BASE, 0] == got[:, 0])   # a build tuple of that key


@pytest.mark.parametrize("name,params", TWO, ids=[p[0] for p in TWO])
def test_inner_poisoned_workspace(name, params):
    # every pairs[] entry must be written by the count pass (empty build
    # partitions, items past a partition's end), never read as allocated
    with phj.Context(0) as fresh:
        fresh.debug_poison_alloc(0xFF)
        check_dup_case(fresh, params, name == "np")


@pytest.mark.parametrize("name,params", TWO, ids=[p[0] for p in TWO])
def test_inner_row_range_limit(ctx, name, params):
    # 65 600^2 = 4 303 360 000 pairs >= 2^32: counted exactly, not materialised
    n = 65_600
    ctx.upload(phj.SIDE_BUILD, with_payloads(np.full(n, 42), R_BASE))
    ctx.upload(phj.SIDE_PROBE, with_payloads(np.full(n, 42), S_BASE))
    assert ctx.join_inner_count(params).matches == n * n
    with pytest.raises(phj.PhjError) as e:
        ctx.join_inner(params)
    assert e.value.code == phj._capi.PHJ_ERR_RANGE
    assert ctx.joined().shape == (0, 3)
    R, S = small_cases()[2]
    hits = S.copy()
    hits[::3, 0] -= 4500   # some of the probe keys now hit
    for S in (S, hits):
        total, rows = expected_inner(R, S)
        ctx.upload(phj.SIDE_BUILD, R)
        ctx.upload(phj.SIDE_PROBE, S)
        assert ctx.join_inner(params).matches == total
        assert np.array_equal(canon(ctx.joined()), rows)
    assert total > 0


def test_inner_group_context_refused():
    with phj.Context(devices=[0, 0], flags=phj.CTX_LOCAL) as g:
        for call in (g.join_inner_count, g.join_inner):
            with pytest.raises(phj.PhjError, match="single-device") as e:
                call(phj.radix_params((8, 8)))
            assert e.value.code == phj._capi.PHJ_ERR_STATE
