"""The batched form of S's pre-aggregating code pass (k_chunk_codes_pipe BATCH,
csrc/phj_partition.h): the sort stage runs once per 4096 KEPT codes, the kept
codes of the input tiles in between waiting in an LDS ring.

Every case forces the pre-aggregation (Context.debug_preagg, as
tests/test_gpu_preagg.py) at |R| = 1M under radix (8, 8): 256 clusters, a
4096-key tile. The count is the oracle's semi-join count and debug_preagg()
shows that the path ran. PHJ_P1_SLOTS (read when the context is created) sets
the workgroups per shard of pass 1: at 1 one workgroup walks every tile of a
shard, closes many batches and then drains; at the default grid a workgroup
sees one to three tiles and only the drain runs. The loop's logic under
interleavings is tests/test_p1_batch_model.py (CPU).
"""
import functools

import numpy as np
import pytest

import partitionedhashjoin_amd as phj
import hashinv
from oracle import oracle as O

pytestmark = pytest.mark.gpu

NR = 1_000_000
NS = 2_000_000
TAIL = 1237          # a partial last tile
T = 4096             # codes of a tile and of a batch
MUR, XXH = phj.HASH_MURMUR3, phj.HASH_XXH3
R_, S_ = phj.SIDE_BUILD, phj.SIDE_PROBE
M64 = (1 << 64) - 1
COUNTER_MUL = 0x9E3779B97F4A7C15   # csrc/phj_hot.h hot_counter_of: (code * this) >> 48


def params(hk=MUR, flags=0):
    p = phj.radix_params((8, 8), hash=hk)
    p.flags |= flags
    return p


@pytest.fixture(scope="module")
def forced(ctx):
    """forced(slots): a context of its own with the pre-aggregation forced and
    PHJ_P1_SLOTS = slots at its creation (0: the default grid)."""
    made = {}

    def get(slots):
        if slots not in made:
            with pytest.MonkeyPatch.context() as mp:
                if slots:
                    mp.setenv("PHJ_P1_SLOTS", str(slots))
                else:
                    mp.delenv("PHJ_P1_SLOTS", raising=False)
                c = phj.Context(0)
            c.debug_preagg(phj.PREAGG_FORCED)
            made[slots] = c
        return made[slots]
    yield get
    for c in made.values():
        c.close()


@functools.lru_cache(maxsize=None)
def zipf_s(alpha, seed=91):
    return O.fill_zipf(NS + TAIL, alpha, 1, NR, seed)


@functools.lru_cache(maxsize=None)
def seq_r(start):
    return O.fill_sequential(NR, start)


@functools.lru_cache(maxsize=None)
def expect_zipf(start, alpha):
    return O.semijoin_count(seq_r(start), zipf_s(alpha))


def run(c, R, S, p, expect=None, columns=False):
    """Upload, join, compare with the oracle; the join's (hot entries, pre-aggregated tuples)."""
    if columns:
        c.upload_columns(R_, R[:, 0], R[:, 1])
        c.upload_columns(S_, S[:, 0], S[:, 1])
    else:
        c.upload(R_, R)
        c.upload(S_, S)
    if expect is None:
        expect = O.semijoin_count(R, S)
    got = c.join(p).matches
    entries, agg = c.debug_preagg()
    assert got == expect, (got, expect, entries, agg)
    assert entries > 0 and 0 < agg <= len(S), (entries, agg)
    return entries, agg


@pytest.mark.parametrize("slots", [1, 0], ids=["one-workgroup", "default-grid"])
@pytest.mark.parametrize("start", [1, 4], ids=["all-hit", "top3-miss"])
@pytest.mark.parametrize("hk", [MUR, XXH], ids=["murmur3", "xxh3"])
@pytest.mark.parametrize("alpha", [1.05, 1.25])
def test_zipf(forced, alpha, hk, start, slots):
    _, agg = run(forced(slots), seq_r(start), zipf_s(alpha), params(hk), expect_zipf(start, alpha))
    assert agg < NS + TAIL   # some codes are kept: batches close (one workgroup) or the drain runs


@pytest.mark.parametrize("slots", [1, 0], ids=["one-workgroup", "default-grid"])
def test_nearly_nothing_hot(forced, slots):
    """One planted key at ~5 % of S over uniform keys (half of them miss): a
    batch closes almost every iteration, the ring at its upper edge."""
    rng = np.random.default_rng(21)
    n = NS + TAIL
    keys = rng.integers(1, 2 * NR + 1, n, dtype=np.int64)
    keys[rng.random(n) < 0.05] = 777_777
    S = O.as_relation(keys)
    _, agg = run(forced(slots), seq_r(1), S, params())
    assert agg <= 0.08 * n


@pytest.mark.parametrize("slots", [1, 0], ids=["one-workgroup", "default-grid"])
@pytest.mark.parametrize("n", [200_000, 3000], ids=["200k", "below-a-tile"])
@pytest.mark.parametrize("hit", [True, False])
def test_everything_hot(forced, hit, n, slots):
    """Single-key S: no batch, an empty drain, the join finds no tiles."""
    c = forced(slots)
    S = O.as_relation(np.full(n, 4242 if hit else NR + 17, dtype=np.int64))
    assert run(c, seq_r(1), S, params()) == (1, n)
    assert c.join(params()).matches == (n if hit else 0)


@functools.lru_cache(maxsize=None)
def cold_keys(hot_key, count):
    """`count` distinct keys of R, each alone on its sample counter and none on
    the hot key's: a counter's representative is its last writer (the hot key's
    must be the hot key), and two cold keys on one counter would count as a
    code sampled twice, which the forced mode's threshold at this size admits."""
    seed = params().hash_seed
    counter = lambda codes: (codes.astype(np.uint64) * np.uint64(COUNTER_MUL)) >> np.uint64(48)
    hot_counter = counter(O.hash_keys(MUR, np.array([hot_key], dtype=np.int64), seed))[0]
    cand = np.arange(10, 10 + 4 * count + 1000, dtype=np.int64) * 3   # every third key: a third of them ...
    ctr = counter(O.hash_keys(MUR, cand, seed))
    _, first = np.unique(ctr, return_index=True)
    cand = cand[np.sort(first)]
    cand = cand[counter(O.hash_keys(MUR, cand, seed)) != hot_counter]
    assert len(cand) >= count and hot_key not in cand
    return cand[:count]


@pytest.mark.parametrize("kept", [T, T + 1, 2 * T - 1, T - 1, 2 * T], ids=lambda k: f"kept{k}")
def test_exact_kept_counts(forced, kept):
    """One hot key plus an exact number of distinct cold keys, one workgroup:
    the ring lands on exactly T (a batch and an empty drain), T + 1, 2T - 1."""
    hot_key, nhot = 5, 60_000
    rng = np.random.default_rng(kept)
    keys = np.concatenate([np.full(nhot, hot_key, dtype=np.int64), cold_keys(hot_key, kept)])
    rng.shuffle(keys)
    S = O.as_relation(keys)
    R = seq_r(1).copy()
    R[R[:, 0] % 6 == 0, 0] += 5_000_000   # ... (the even ones) then miss
    entries, agg = run(forced(1), R, S, params())
    assert (entries, agg) == (1, nhot)     # so the workgroups keep exactly `kept` codes


def test_cold_codes_in_one_cluster(forced):
    """Every kept code in one cluster, three workgroups: one long chain, a chunk
    start in most batches, waits on other workgroups' batch publishes."""
    p = params()
    rng = np.random.default_rng(33)
    codes = {(int(rng.integers(0, 1 << 63)) & ~0xFF00) | (0x5A << 8) for _ in range(6000)}   # the digit is bits 8..15
    crowd = np.array([hashinv.preimage(True, c, p.hash_seed) for c in sorted(codes)], dtype=np.int64)
    n = 600_000 + 321
    pick = rng.random(n)
    keys = crowd[rng.integers(0, len(crowd), n)]
    keys[pick < 0.4] = 31_337             # the planted hot key
    S = O.as_relation(keys)
    R = np.concatenate([seq_r(1), O.as_relation(crowd[::2])])   # every other crowd key has a partner
    _, agg = run(forced(3), R, S, p)
    assert agg <= 0.5 * n                 # the crowd's cluster has four entries: the rest is kept


def test_key_columns(forced):
    """The key-column form of the pass on one Zipf case (bound as
    tests/test_gpu_columns.py binds them): COLS 1, 8-B loads."""
    c = forced(1)
    run(c, seq_r(4), zipf_s(1.05), params(), expect_zipf(4, 1.05), columns=True)
    assert c.relation_info(S_).packed == 0
    run(c, seq_r(1), zipf_s(1.25), params(XXH), expect_zipf(1, 1.25), columns=True)


@pytest.mark.parametrize("slots", [1, 0], ids=["one-workgroup", "default-grid"])
def test_back_to_back(forced, slots):
    """Two joins on one context, both exact: the state the previous join's tail cleared."""
    c = forced(slots)
    timed = params(flags=phj.DEFER_TIMERS | phj.LEAN_TIMERS)
    run(c, seq_r(4), zipf_s(1.25), timed, expect_zipf(4, 1.25))
    run(c, seq_r(1), zipf_s(1.05), timed, expect_zipf(1, 1.05))
    assert c.join(timed).matches == expect_zipf(1, 1.05)
    c.timers_report()
