"""The hot weights resolved by a kernel of their own (csrc/phj_hot.h k_hot_resolve).

S's pass 1 counts the hot keys into their entries' weights; after it one
workgroup per cluster scans the cluster's R codes through R's pass-1 tile list
and adds the weights of the entries it meets to the count, and R's chain runs
on the aux stream beside the hot-key prologue. The cases here are the ones
that kernel and that schedule can get wrong: clusters that have no S tile left,
a hot key R holds in tiles far apart, a cluster beyond the LDS limit, an empty
build side, R replaced between back-to-back joins, and a table ignored for low
mass. Every count is the oracle's semi-join count, and every case asserts from
debug_preagg() whether the path ran.
"""
import functools

import numpy as np
import pytest

import partitionedhashjoin_amd as phj
import hashinv
from oracle import oracle as O

pytestmark = pytest.mark.gpu

NR = 1_000_000
MUR = phj.HASH_MURMUR3
M64 = (1 << 64) - 1
COUNTER_MUL = 0x9E3779B97F4A7C15   # csrc/phj_hot.h hot_counter_of: (code * this) >> 48
CL_LIM = 16384 // 4 * 3            # csrc/phj_cluster.h cl_lim(kClCapMax): R codes of a cluster with an LDS table


def params(flags=0):
    p = phj.radix_params((8, 8), hash=MUR)
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
def seq_r(start, n=NR):
    return O.fill_sequential(n, start)


def codes_of(p, keys):
    return O.hash_keys(p.hash, keys, p.hash_seed)


def cluster_of(codes):
    """|R| = 1M under radix (8, 8): 256 clusters, the digit is bits 8..15 of the code."""
    return (np.asarray(codes, dtype=np.uint64) >> np.uint64(8)) & np.uint64(0xFF)


def counter_of(codes):
    return (np.asarray(codes, dtype=np.uint64) * np.uint64(COUNTER_MUL)) >> np.uint64(48)


def crafted(p, rng, cluster, n):
    """n distinct keys whose codes fall in `cluster`."""
    codes = {(int(rng.integers(0, 1 << 63)) & ~0xFF00) | (cluster << 8) for _ in range(n + 8)}
    codes = sorted(codes)[:n]
    keys = np.array([hashinv.preimage(True, c, p.hash_seed) for c in codes], dtype=np.int64)
    assert len(np.unique(keys)) == n and (cluster_of(codes_of(p, keys)) == cluster).all()
    return keys


def skewed_s(p, rng, n, hot_keys, share, keep_out=()):
    """n probe keys: each hot key `share` of them, the rest uniform over R's
    sequential keys outside the clusters `keep_out` and off the hot keys'
    sample counters (so the sample's representative of those is the hot key)."""
    cold = rng.integers(1, NR + 1, n, dtype=np.int64)
    cc = codes_of(p, cold)
    bad = np.isin(cluster_of(cc), np.array(keep_out, dtype=np.uint64)) | \
        np.isin(counter_of(cc), counter_of(codes_of(p, hot_keys)))
    good = cold[~bad]
    cold[bad] = good[np.arange(int(bad.sum())) % len(good)]
    pick = rng.random(n)
    nhot = 0
    for j, k in enumerate(hot_keys):
        m = (pick >= share * j) & (pick < share * (j + 1))
        cold[m] = k
        nhot += int(m.sum())
    return O.as_relation(cold), nhot


def run(c, R, S, p, ran=True, upload_s=True):
    """Upload, join, compare with the oracle; returns the join's statistics."""
    c.upload(phj.SIDE_BUILD, R)
    if upload_s:
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


@pytest.mark.parametrize("in_r", [3, 1], ids=["all-in-R", "one-in-R"])
def test_clusters_without_s_tiles(hot, in_r):
    """Three hot keys in three clusters whose every S tuple is one of them: all
    of it is pre-aggregated, the clusters have no S tile, k_hot_resolve alone counts them."""
    p = params()
    rng = np.random.default_rng(21)
    clusters = (0x11, 0x5A, 0xC3)
    keys = np.concatenate([crafted(p, rng, cl, 1) for cl in clusters])
    S, nhot = skewed_s(p, rng, 1_500_000 + 411, keys, 0.1, keep_out=clusters)
    R = np.concatenate([seq_r(1), O.as_relation(keys[:in_r])])
    _, agg = run(hot, R, S, p)
    assert agg >= nhot   # the hot keys are off every other key's sample counter: all three were entered


def test_hot_key_copies_far_apart(hot):
    """R holds the hottest key in its first, a middle and its last tile (different shards): counted once."""
    S = O.fill_zipf(2_000_000 + 99, 1.05, 1, NR, 31)
    R = seq_r(1).copy()
    assert R[0, 0] == 1
    R[NR // 2, 0] = 1
    R[NR - 1, 0] = 1
    run(hot, R, S, params())


def test_big_cluster_with_hot_entries(hot):
    """A cluster beyond the LDS limit (CL_LIM + 1 crafted R keys on top of its
    share of the sequential ones: the HBM table, more runs than a build reads)
    with two hot S keys, one with a partner and one without."""
    p = params()
    rng = np.random.default_rng(41)
    crowd = crafted(p, rng, 0x5A, CL_LIM + 2)
    with_partner, without = crowd[0], crowd[-1]
    S, _ = skewed_s(p, rng, 1_500_000 + 7, np.array([with_partner, without]), 0.1)
    R = np.concatenate([seq_r(1), O.as_relation(crowd[:-1])])
    assert int((cluster_of(codes_of(p, R[:, 0])) == 0x5A).sum()) > CL_LIM
    run(hot, R, S, p)


def test_empty_build_side_then_a_normal_join(hot):
    S = O.fill_zipf(1_500_000 + 5, 1.25, 1, NR, 51)
    hot.upload(phj.SIDE_BUILD, O.relation(0))
    hot.upload(phj.SIDE_PROBE, S)
    assert hot.join(params()).matches == 0
    run(hot, seq_r(1), S, params())


def test_back_to_back_with_r_replaced(hot):
    """Joins under the bench's timer flags with R replaced in between (shifted
    starts, one of another size: the tile list changes size), then a plain one:
    a stale tile list, a wrong clear of R's chunk state or an aux stream that
    did not wait for the join before would show as a wrong count."""
    timed = params(flags=phj.DEFER_TIMERS | phj.LEAN_TIMERS)
    S = O.fill_zipf(2_000_000 + 55, 1.05, 1, NR, 61)
    hot.upload(phj.SIDE_PROBE, S)
    for start, n in [(1, NR), (4, NR), (1, 700_000), (1, NR)]:
        run(hot, seq_r(start, n), S, timed, upload_s=False)
    run(hot, seq_r(4), S, params(), upload_s=False)
    hot.timers_report()


def test_table_ignored_for_low_mass(ctx):
    """Auto mode at the size floor, skew 0.5: whatever the first look and the
    sample find covers too little, S's pass and k_hot_resolve ignore the table."""
    S = O.fill_zipf(32 * 128 * 4096, 0.5, 1, NR, 71)
    run(ctx, seq_r(1), S, params(), ran=False)
