"""Hot-key pre-aggregation of the counting LDS join (csrc/phj_hot.h).

phj_join samples the probe side, counts its hottest keys in S's pass 1 instead
of writing them and resolves them against R inside R's pass 1. Whatever the
sample selects, the count is the oracle's semi-join count. The debug entry
(Context.debug_preagg) forces the path at these small shapes and reports the
last join's (hot entries, pre-aggregated tuples); every case asserts from
those that the path ran (or, where it must be off, that it did not).
"""
import functools

import numpy as np
import pytest

import partitionedhashjoin_amd as phj
import hashinv
from oracle import oracle as O

pytestmark = pytest.mark.gpu

NR = 1_000_000
NS = 3_000_000
TAIL = 1237          # a partial last tile
MUR = phj.HASH_MURMUR3
XXH = phj.HASH_XXH3
M64 = (1 << 64) - 1
COUNTER_MUL = 0x9E3779B97F4A7C15   # csrc/phj_hot.h hot_counter_of: (code * this) >> 48


def params(hk=MUR, flags=0):
    p = phj.radix_params((8, 8), hash=hk)
    p.flags |= flags
    return p


@pytest.fixture(scope="module")
def hot(ctx):
    """A context of its own in forced mode (the session's stays in auto)."""
    c = phj.Context(0)
    c.debug_preagg(phj.PREAGG_FORCED)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def zipf_s(alpha, seed=77):
    return O.fill_zipf(NS + TAIL, alpha, 1, NR, seed)


@functools.lru_cache(maxsize=None)
def seq_r(start):
    return O.fill_sequential(NR, start)


def run(c, R, S, p, ran=True):
    """Upload, join, compare with the oracle; returns the join's statistics."""
    c.upload(phj.SIDE_BUILD, R)
    c.upload(phj.SIDE_PROBE, S)
    expect = O.semijoin_count(R, S)
    got = c.join(p).matches
    entries, agg = c.debug_preagg()
    assert got == expect, (got, expect, entries, agg)
    if ran:
        assert entries > 0 and 0 < agg <= len(S), (entries, agg)
    else:
        assert (entries, agg) == (0, 0)
    return entries, agg


@pytest.mark.parametrize("start", [1, 4], ids=["all-hit", "top3-miss"])
@pytest.mark.parametrize("hk", [MUR, XXH], ids=["murmur3", "xxh3"])
@pytest.mark.parametrize("alpha", [1.05, 1.25])
@pytest.mark.parametrize("tail", [0, TAIL])
def test_zipf(hot, tail, alpha, hk, start):
    S = zipf_s(alpha)[:NS + tail]
    run(hot, seq_r(start), S, params(hk))


@pytest.mark.parametrize("n", [200_000, 3000], ids=["200k", "below-a-tile"])
@pytest.mark.parametrize("hit", [True, False])
def test_single_key(hot, hit, n):
    R = seq_r(1)
    S = O.as_relation(np.full(n, 4242 if hit else NR + 17, dtype=np.int64))
    entries, agg = run(hot, R, S, params())
    # everything pre-aggregated: pass 1 writes nothing, the join has no tiles
    assert (entries, agg) == (1, n)
    assert hot.join(params()).matches == (n if hit else 0)


def test_duplicate_build_keys(hot):
    S = zipf_s(1.05)[:NS]
    R = seq_r(1).copy()
    R[1000:1003, 0] = 1     # the hottest key three times (keys 1001-1003 leave R)
    R[2000:2002, 0] = 2
    run(hot, R, S, params())


def codes_to_keys(p, codes):
    mur = p.hash == MUR
    return np.array([hashinv.preimage(mur, int(c), p.hash_seed) for c in codes], dtype=np.int64)


@pytest.mark.parametrize("hk", [MUR, XXH], ids=["murmur3", "xxh3"])
def test_set_overflow(hot, hk):
    """12 keys of one cluster (which has four entries: two 2-way sets), each ~5 % of S."""
    p = params(hk)
    rng = np.random.default_rng(5)
    # |R| = 1M: 256 clusters, the digit is bits 8..15 of the code
    codes = [(int(rng.integers(0, 1 << 63)) & ~0xFF00) | (0x5A << 8) for _ in range(12)]
    crowd = codes_to_keys(p, codes)
    n = 1_500_000 + 321
    keys = rng.integers(1, NR + 1, n, dtype=np.int64)
    pick = rng.random(n)
    for j, k in enumerate(crowd):
        keys[(pick >= 0.05 * j) & (pick < 0.05 * (j + 1))] = k
    S = O.as_relation(keys)
    R = np.concatenate([seq_r(1), O.as_relation(crowd[::2])])   # every other crowd key has a partner
    _, agg = run(hot, R, S, p)
    assert agg <= n - 8 * 0.04 * n   # the crowd's cluster has four entries: eight of the twelve stay on the normal path


def test_sample_counter_collisions(hot):
    """Cold keys that share a hot key's sample counter are selected with it."""
    p = params()
    rng = np.random.default_rng(9)
    inv = pow(COUNTER_MUL, -1, 1 << 64)
    top = int(rng.integers(0, 1 << 16))
    codes = [(((top << 48) | int(rng.integers(0, 1 << 48))) * inv) & M64 for _ in range(301)]
    assert {((c * COUNTER_MUL) & M64) >> 48 for c in codes} == {top}
    ks = codes_to_keys(p, codes)
    hot_key, cold = ks[0], ks[1:]
    n = 1_000_000 + 77
    keys = rng.integers(1, NR + 1, n, dtype=np.int64)
    pick = rng.random(n)
    keys[pick < 0.05] = hot_key
    slots = np.flatnonzero((pick >= 0.05) & (pick < 0.06))
    keys[slots] = cold[np.arange(len(slots)) % len(cold)]   # ~33 tuples of each cold key
    S = O.as_relation(keys)
    R = np.concatenate([seq_r(1), O.as_relation(np.concatenate([[hot_key], cold[::2]]))])
    run(hot, R, S, p)
    R = np.concatenate([seq_r(1), O.as_relation(cold[1::2])])   # the hot key misses
    run(hot, R, S, p)


def test_back_to_back_no_stale_state(hot):
    """Three joins under the bench's timer flags, S regenerated between them
    (the first leaves unconsumed weights: its hottest keys miss), then a plain one."""
    timed = params(flags=phj.DEFER_TIMERS | phj.LEAN_TIMERS)
    n = 2_000_000 + 55
    for i, (alpha, seed, start) in enumerate([(1.25, 11, 4), (1.05, 12, 1), (0.5, 13, 1), (1.05, 14, 2)]):
        S = O.fill_zipf(n, alpha, 1, NR, seed)
        run(hot, seq_r(start), S, timed if i < 3 else params())
    hot.timers_report()


@pytest.mark.parametrize("env", [{"PHJ_R_CHUNK": "0"}, {"PHJ_R_ORDER": "0"}, {"PHJ_R_ORDER": "2"}],
                         ids=lambda e: ",".join(f"{k[4:]}={v}" for k, v in e.items()))
def test_other_schedules_are_off(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with phj.Context(0) as c:
        c.debug_preagg(phj.PREAGG_FORCED)
        run(c, seq_r(4), zipf_s(1.05)[:NS], params(), ran=False)


def test_group_context_is_off():
    S = zipf_s(1.05)[:NS]
    R = seq_r(4)
    with phj.Context(devices=[0] * 3, flags=phj.CTX_LOCAL) as g:
        g.debug_preagg(phj.PREAGG_FORCED)
        run(g, R, S, params(), ran=False)


def test_off_means_off(hot):
    S = zipf_s(1.25)[:NS + TAIL]
    R = seq_r(4)
    forced = run(hot, R, S, params())
    assert forced[1] > 0
    hot.debug_preagg(phj.PREAGG_OFF)
    try:
        hot.upload(phj.SIDE_PROBE, S)
        off = hot.join(params()).matches
        assert hot.debug_preagg() == (0, 0)
        assert off == O.semijoin_count(R, S)
    finally:
        hot.debug_preagg(phj.PREAGG_FORCED)


def test_auto_is_off_below_the_size_floor(ctx):
    run(ctx, seq_r(1), zipf_s(1.05)[:NS], params(), ran=False)
