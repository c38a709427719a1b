"""The front of the batched loop of S's pre-aggregating code pass
(k_chunk_codes_pipe BATCH, csrc/phj_partition.h): key loads, the full-tile
form of the lookups and the append, and the append's wave-uniform fast path,
at the smallest shapes where each can go wrong.

Set up as tests/test_gpu_p1_batch.py: contexts of their own with the
pre-aggregation forced, |R| = 1M under radix (8, 8) (256 clusters, a 4096-key
tile), PHJ_P1_SLOTS 1 (one workgroup walks every tile, closes batches, drains)
and the default grid. Counts are the oracle's semi-join counts and
debug_preagg() shows that the path ran.

A forced hot table takes the codes sampled at least twice, so a probe side of
one tuple has no hot entry: that one size runs the per-tile loop over the same
loads (debug_preagg() then reads (0, 0)), and is checked for its count alone.
"""
import functools

import numpy as np
import pytest

import partitionedhashjoin_amd as phj
from oracle import oracle as O

pytestmark = pytest.mark.gpu

NR = 1_000_000
T = 4096
MUR, XXH = phj.HASH_MURMUR3, phj.HASH_XXH3
R_, S_ = phj.SIDE_BUILD, phj.SIDE_PROBE
I64_MIN = -(1 << 63)
SPECIAL = np.array([0, -1, I64_MIN], dtype=np.int64)
COUNTER_MUL = 0x9E3779B97F4A7C15   # csrc/phj_hot.h hot_counter_of: (code * this) >> 48
HOT_KEY = 5


def params(hk=MUR):
    return phj.radix_params((8, 8), hash=hk)


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
def seq_r(n=NR, start=1):
    return O.fill_sequential(n, start)


@functools.lru_cache(maxsize=None)
def r_with_special(with_special):
    R = seq_r()
    return np.concatenate([R, O.as_relation(SPECIAL)]) if with_special else R


def join_checked(c, R, S, p, ran=True, columns=False):
    if columns:
        c.upload_columns(R_, R[:, 0], R[:, 1])
        c.upload_columns(S_, S[:, 0], S[:, 1])
    else:
        c.upload(R_, R)
        c.upload(S_, S)
    expect = O.semijoin_count(R, S)
    got = c.join(p).matches
    entries, agg = c.debug_preagg()
    assert got == expect, (got, expect, entries, agg)
    if ran:
        assert entries > 0 and 0 < agg <= len(S), (entries, agg)
    else:
        assert (entries, agg) == (0, 0)
    return entries, agg


# ---- tile edges: the loads past the relation's end, the full-tile form ----

def edge_keys(n):
    """n keys: the hot key, with 0, -1 and INT64_MIN at the start and again
    before the last key, which is a key of R that occurs once. A lane past the
    end that read 0, or the last tuple again, would count once more."""
    keys = np.full(n, HOT_KEY, dtype=np.int64)
    keys[:3] = SPECIAL[:min(3, n)]
    if n >= 8:
        keys[n - 4:n - 1] = SPECIAL
        keys[n - 1] = 12_345
    return keys


@pytest.mark.parametrize("slots", [1, 0], ids=["one-workgroup", "default-grid"])
@pytest.mark.parametrize("with_special", [True, False], ids=["special-in-R", "special-not-in-R"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4095, 4096, 4097, 3 * T, 3 * T + 1, 3 * T + 4095])
def test_tile_edges(forced, n, with_special, slots):
    S = O.as_relation(edge_keys(n))
    join_checked(forced(slots), r_with_special(with_special), S, params(), ran=n > 1)


@pytest.mark.parametrize("n", [4097, 3 * T + 4095])
def test_tile_edges_xxh3(forced, n):
    join_checked(forced(1), r_with_special(True), O.as_relation(edge_keys(n)), params(XXH))


# ---- straddling waves: the append's fast path and the wave that crosses the batch's end ----

@functools.lru_cache(maxsize=None)
def cold_keys(count):
    """`count` distinct keys of R, each alone on its sample counter and none on
    the hot key's (tests/test_gpu_p1_batch.py cold_keys: two cold keys on one
    counter would count as a code sampled twice, which the forced threshold admits)."""
    seed = params().hash_seed
    counter = lambda codes: (codes.astype(np.uint64) * np.uint64(COUNTER_MUL)) >> np.uint64(48)
    hot_counter = counter(O.hash_keys(MUR, np.array([HOT_KEY], dtype=np.int64), seed))[0]
    cand = np.arange(10, 10 + 4 * count + 1000, dtype=np.int64) * 3
    ctr = counter(O.hash_keys(MUR, cand, seed))
    _, first = np.unique(ctr, return_index=True)
    cand = cand[np.sort(first)]
    cand = cand[counter(O.hash_keys(MUR, cand, seed)) != hot_counter]
    assert len(cand) >= count and HOT_KEY not in cand
    return cand[:count]


@functools.lru_cache(maxsize=None)
def half_miss_r():
    R = seq_r().copy()
    R[R[:, 0] % 6 == 0, 0] += 5_000_000   # every other cold key (multiples of 3) then misses
    return R


def kept_layout(kept, per_tile, at_end):
    """Whole tiles of the hot key with `per_tile` cold keys at the start (wave
    0's elements) or the end (wave 15's) of each, `kept` cold keys in all."""
    ntiles = (kept + per_tile - 1) // per_tile
    keys = np.full(ntiles * T, HOT_KEY, dtype=np.int64)
    cold = cold_keys(kept)
    for j in range(ntiles):
        c = cold[j * per_tile:(j + 1) * per_tile]
        lo = (j + 1) * T - len(c) if at_end else j * T
        keys[lo:lo + len(c)] = c
    return keys


@pytest.mark.parametrize("at_end", [False, True], ids=["wave0", "wave15"])
@pytest.mark.parametrize("kept", [T - 1, T, T + 1, T + 63, T + 64, T + 65, 2 * T - 1, 2 * T, 2 * T + 1],
                         ids=lambda k: f"kept{k}")
def test_batch_boundary_inside_a_wave(forced, kept, at_end):
    """200 kept codes per tile, all in one wave: 4096 = 20 * 200 + 96, so the
    batch's end falls inside that wave's kept codes of the 21st tile, and the
    second batch's inside the 41st's."""
    keys = kept_layout(kept, 200, at_end)
    entries, agg = join_checked(forced(1), half_miss_r(), O.as_relation(keys), params())
    assert (entries, agg) == (1, len(keys) - kept)   # so the workgroup keeps exactly `kept` codes


@pytest.mark.parametrize("at_end", [False, True], ids=["wave0-all-wave15-none", "wave15-all-wave0-none"])
def test_whole_wave_kept_or_dropped(forced, at_end):
    """256 cold keys per tile: one wave keeps every code of its four items, the
    fifteen others keep none; the batch's end meets a tile's end."""
    kept = T + 256 + 17
    keys = kept_layout(kept, 256, at_end)
    entries, agg = join_checked(forced(1), half_miss_r(), O.as_relation(keys), params())
    assert (entries, agg) == (1, len(keys) - kept)


# ---- key columns ----

@pytest.mark.parametrize("n", [4097, 3 * T + 4095, 200_001])
def test_columns_odd_length(forced, n):
    join_checked(forced(1), r_with_special(True), O.as_relation(edge_keys(n)), params(), columns=True)
    assert forced(1).relation_info(S_).packed == 0


@pytest.mark.parametrize("slots", [1, 0], ids=["one-workgroup", "default-grid"])
def test_column_view_one_element_into_a_buffer(forced, slots):
    """The key column is a view one element into a buffer: its base is 8-byte
    but not 16-byte aligned, the element before it and those behind it are
    keys of R (an over-read raises the count), and its length is odd."""
    c = forced(slots)
    n = 3 * T + 4095
    real = edge_keys(n)
    R = r_with_special(True)
    donor = phj.Context(0)
    donor.upload_columns(S_, np.concatenate([[7], real, np.full(T + 3, 7)]).astype(np.int64))
    base = donor.columns_ptr(S_)[0]
    assert base % 16 == 0
    c.upload_columns(R_, R[:, 0])
    c.bind_columns(S_, base + 8, None, n, keepalive=donor)
    for hk in (MUR, XXH):
        got = c.join(params(hk)).matches
        entries, agg = c.debug_preagg()
        assert got == O.semijoin_count(R, O.as_relation(real)), (got, entries, agg)
        assert entries > 0 and 0 < agg <= n
    c.upload_columns(S_, real[:1])   # (rebinding releases the donor)
    donor.close()


# ---- R's side: the plain forms of the pass run the same loads ----

@pytest.mark.parametrize("slots", [1, 0], ids=["one-workgroup", "default-grid"])
@pytest.mark.parametrize("nr", [4097, 8 * T + 1])
def test_small_r(forced, nr, slots):
    """R of one tuple more than whole tiles (the LDS join reads R by tiles of
    the code pass), against a small S: the hot key hits, keys past R miss."""
    rng = np.random.default_rng(nr)
    keys = rng.integers(1, 2 * nr + 1, 3 * T + 17, dtype=np.int64)
    keys[rng.random(len(keys)) < 0.5] = nr          # R's last key, hot
    keys[:3] = SPECIAL
    R = seq_r(nr)
    join_checked(forced(slots), R, O.as_relation(keys), params())
    join_checked(forced(slots), np.concatenate([R, O.as_relation(SPECIAL)]), O.as_relation(keys), params(XXH))


# ---- beyond 4 GiB: the tile's base is a 64-bit address ----

def test_probe_side_beyond_4gib(forced):
    import torch
    ns = (1 << 28) + T + 5
    need = 16 * ns + 8 * ns + (3 << 30)   # the tuples, their codes, pools and tables
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip(f"needs {need / 2**30:.1f} GiB of free device memory, {free / 2**30:.1f} GiB free")
    c = forced(0)
    start = 4                                      # R = [4, NR + 3]: S's keys 1..3, the hottest, miss
    c.generate_sequential(R_, NR, start)
    c.generate_zipf(S_, ns, 1.05, 1, NR, 20240521)
    expect = c.count_in_range(S_, start, NR)
    got = c.join(params()).matches
    entries, agg = c.debug_preagg()
    assert got == expect, (got, expect, entries, agg)
    assert entries > 0 and 0 < agg < ns
    c.upload(S_, O.as_relation(edge_keys(8)))      # release the 4 GiB
