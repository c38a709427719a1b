"""The hot weights resolved inside the LDS join, and the two-launch prologue.

A hot entry is a probe code that carries a weight: the workgroup of
k_cluster_probe that owns a cluster (its tile range holds the cluster's first
S tile) looks the cluster's entries up in the LDS table it has just built, and
k_cluster_probe_big takes the clusters that kernel never builds (an HBM
table, or no S tile left). The prologue is one sample launch whose workgroups
vote from their own LDS counts, and a selection that leaves the state clean
for the next join (csrc/phj_hot.h, csrc/phj_cluster.h). The cases here are
what that ownership rule and that clean-state bookkeeping can get wrong; the
shapes and helpers are test_gpu_preagg_resolve.py's (|R| = 1M under radix
(8, 8): 256 clusters). Every count is the oracle's semi-join count, and every
case asserts from debug_preagg() whether the path ran.
"""
import functools

import numpy as np
import pytest

import partitionedhashjoin_amd as phj
import hashinv
from oracle import oracle as O
from test_gpu_preagg_resolve import CL_LIM, NR, cluster_of, codes_of, counter_of, crafted, params, run, seq_r, skewed_s

pytestmark = pytest.mark.gpu

FLOOR = 32 * 128 * 4096   # csrc/phj_capi.hip kHotMinS: auto mode's smallest S


@pytest.fixture(scope="module")
def hot(ctx):
    """A context of its own in forced mode (the session's stays in auto)."""
    c = phj.Context(0)
    c.debug_preagg(phj.PREAGG_FORCED)
    yield c
    c.close()


def crafted_top(p, rng, cluster, n):
    """n distinct keys of `cluster` whose codes have the top bit set: the
    cluster's other hot set (crafted()'s codes all have it clear)."""
    codes = sorted({(int(rng.integers(0, 1 << 63)) & ~0xFF00) | (cluster << 8) | (1 << 63) for _ in range(n + 8)})[:n]
    keys = np.array([hashinv.preimage(True, c, p.hash_seed) for c in codes], dtype=np.int64)
    assert len(np.unique(keys)) == n and (cluster_of(codes_of(p, keys)) == cluster).all()
    return keys


def test_cluster_spread_over_many_workgroups(hot):
    """Cluster 0x5A gets ~200K cold S tuples (25000 crafted keys, 8 copies
    each: about 49 tiles against ~3 per probe workgroup, so some twenty
    workgroups build its table) and two hot keys, one with a partner in R and
    one without: only the workgroup holding the cluster's first tile may add
    the weight. The cold keys' codes have the top bit clear and the hot keys'
    have it set, so the two are the only candidates of their set: both are entered."""
    p = params()
    rng = np.random.default_rng(101)
    cold = crafted(p, rng, 0x5A, 25000)
    hot_keys = crafted_top(p, rng, 0x5A, 2)
    cold = cold[~np.isin(counter_of(codes_of(p, cold)), counter_of(codes_of(p, hot_keys)))]
    S, nhot = skewed_s(p, rng, 1_500_000 + 13, hot_keys, 0.1, keep_out=(0x5A,))
    S = np.concatenate([S, O.as_relation(np.repeat(cold, 8))])
    S = S[rng.permutation(len(S))]
    R = np.concatenate([seq_r(1), O.as_relation(cold[::4]), O.as_relation(hot_keys[:1])])
    assert int((cluster_of(codes_of(p, R[:, 0])) == 0x5A).sum()) <= CL_LIM
    _, agg = run(hot, R, S, p)
    assert agg >= nhot   # both hot keys were entered


@pytest.mark.parametrize("start", [1, 4])
def test_range_boundaries_across_cluster_starts(hot, start):
    """S of n and n + 4096 k tuples (prefixes of one Zipf 1.05 draw): every
    probe workgroup's range boundary moves across the clusters' first tiles,
    so a range starts inside a cluster at one size and on its first tile at another."""
    n = 1_500_000 + 77
    S = O.fill_zipf(n + 4096 * 7, 1.05, 1, NR, 111)
    R = seq_r(start)
    hot.upload(phj.SIDE_BUILD, R)
    for k in (0, 1, 2, 7):
        Sk = S[:n + 4096 * k]
        hot.upload(phj.SIDE_PROBE, Sk)
        expect = O.semijoin_count(R, Sk)
        got = hot.join(params()).matches
        entries, agg = hot.debug_preagg()
        assert got == expect, (k, got, expect, entries, agg)
        assert entries > 0 and 0 < agg <= len(Sk), (k, entries, agg)


@pytest.mark.parametrize("in_r", [(1, 0, 1, 0), (0, 1, 0, 1), (1, 1, 1, 1)], ids=["even-in-R", "odd-in-R", "all-in-R"])
def test_tile_less_clusters_at_the_edges(hot, in_r):
    """Clusters 0 (its empty value is not 0), 0x7E and 0x7F (adjacent) and 255
    (its tile position equals the total) keep no S tile: each has one hot key
    and no other S tuple; some of the keys are in R and some are not."""
    p = params()
    rng = np.random.default_rng(121)
    clusters = (0x00, 0x7E, 0x7F, 0xFF)
    keys = np.concatenate([crafted(p, rng, cl, 1) for cl in clusters])
    S, nhot = skewed_s(p, rng, 1_500_000 + 411, keys, 0.1, keep_out=clusters)
    R = np.concatenate([seq_r(1), O.as_relation(keys[np.array(in_r, dtype=bool)])])
    _, agg = run(hot, R, S, p)
    assert agg >= nhot


def test_big_and_tile_less_cluster(hot):
    """Cluster 0x5A is beyond the LDS limit (CL_LIM + 1 crafted R keys on top of
    its share of the sequential ones) and every S tuple of it is hot, one key
    with a partner and one without: an HBM table and no S tile."""
    p = params()
    rng = np.random.default_rng(131)
    crowd = crafted(p, rng, 0x5A, CL_LIM + 2)
    hot_keys = np.array([crowd[0], crowd[-1]])
    S, nhot = skewed_s(p, rng, 1_500_000 + 7, hot_keys, 0.1, keep_out=(0x5A,))
    R = np.concatenate([seq_r(1), O.as_relation(crowd[:-1])])
    assert int((cluster_of(codes_of(p, R[:, 0])) == 0x5A).sum()) > CL_LIM
    assert int((cluster_of(codes_of(p, S[:, 0])) == 0x5A).sum()) == nhot
    _, agg = run(hot, R, S, p)
    assert agg >= nhot


@functools.lru_cache(maxsize=None)
def sequence_inputs():
    """The back-to-back sequence's inputs and counts, computed once."""
    skewed = O.fill_zipf(1_500_000 + 55, 1.05, 1, NR, 141)
    uniform = O.as_relation(np.random.default_rng(142).integers(1, NR + 1, 1_500_000 + 3, dtype=np.int64))
    small = seq_r(1, 100_000)
    steps = [   # (mode, R, S, the path ran)
        (phj.PREAGG_FORCED, seq_r(1), skewed, True),
        (phj.PREAGG_OFF, seq_r(1), skewed, False),
        (phj.PREAGG_FORCED, seq_r(4), skewed, True),
        (phj.PREAGG_FORCED, seq_r(4), uniform, True),   # (forced: a key sampled twice is entered)
        (phj.PREAGG_FORCED, small, uniform, None),      # R of 100K: another cluster count (or another join)
        (phj.PREAGG_FORCED, seq_r(1), uniform, True),
        (phj.PREAGG_FORCED, seq_r(1), skewed, True),
    ]
    return [(m, R, S, ran, O.semijoin_count(R, S)) for m, R, S, ran in steps]


def run_sequence(c, p):
    for i, (mode, R, S, ran, expect) in enumerate(sequence_inputs()):
        c.debug_preagg(mode)
        c.upload(phj.SIDE_BUILD, R)
        c.upload(phj.SIDE_PROBE, S)
        got = c.join(p).matches
        entries, agg = c.debug_preagg()
        assert got == expect, (i, got, expect, entries, agg)
        if ran is None:   # whichever join this size takes: consistent statistics
            assert (entries, agg) == (0, 0) or (entries > 0 and 0 < agg <= len(S)), (i, entries, agg)
        elif ran:
            assert entries > 0 and 0 < agg <= len(S), (i, entries, agg)
        else:
            assert (entries, agg) == (0, 0), (i, entries, agg)


@pytest.mark.parametrize("poison", [None, 0xA5], ids=["plain-alloc", "poisoned-alloc"])
def test_back_to_back_without_a_steady_state_clear(poison):
    """One context, no k_hot_clear between joins: the selection leaves the
    counters and control words clean, the host clears only when the state is
    not known to be (first join, another cluster count). Forced skewed S, off,
    forced again, a uniform S, R of 100K, back to 1M; under the bench's timer
    flags and under plain ones; and again with every new buffer poisoned."""
    c = phj.Context(0)
    try:
        if poison is not None:
            c.debug_poison_alloc(poison)
        run_sequence(c, params(flags=phj.DEFER_TIMERS | phj.LEAN_TIMERS))
        c.timers_report()
        run_sequence(c, params())
    finally:
        c.close()


def mixed_s():
    """First half uniform, second half 30 % one key: some sample workgroups see skew and some do not."""
    rng = np.random.default_rng(153)
    keys = rng.integers(1, NR + 1, FLOOR, dtype=np.int64)
    tail = keys[FLOOR // 2:]
    tail[rng.random(len(tail)) < 0.3] = 4242
    return O.as_relation(keys)


@pytest.mark.parametrize("kind", ["zipf", "uniform", "mixed"])
def test_auto_mode_at_the_size_floor(ctx, kind):
    """Auto mode's smallest S: Zipf 1.05 turns the path on, uniform keys leave
    no vote and an empty table, and with votes from only half of the sample
    workgroups the count is exact whichever way the table falls."""
    if kind == "zipf":
        S = O.fill_zipf(FLOOR, 1.05, 1, NR, 151)
    elif kind == "uniform":
        S = O.as_relation(np.random.default_rng(152).integers(1, NR + 1, FLOOR, dtype=np.int64))
    else:
        S = mixed_s()
    R = seq_r(1)
    ctx.upload(phj.SIDE_BUILD, R)
    ctx.upload(phj.SIDE_PROBE, S)
    expect = O.semijoin_count(R, S)
    got = ctx.join(params()).matches
    entries, agg = ctx.debug_preagg()
    assert got == expect, (got, expect, entries, agg)
    if kind == "zipf":
        assert entries > 0 and 0 < agg <= len(S), (entries, agg)
    elif kind == "uniform":
        assert (entries, agg) == (0, 0)
    else:
        assert (entries, agg) == (0, 0) or (entries > 0 and 0 < agg <= len(S)), (entries, agg)
