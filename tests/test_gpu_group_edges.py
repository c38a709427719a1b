"""The multi-GPU member step (csrc/phj_group.h member_radix / member_nopart)
on crafted codes, empty shards and 16 ranks.

A group of `world` members on device 0 (PHJ_CTX_LOCAL, worlds 2, 3 and 16)
runs what nothing else runs: the multi-segment kernels (cl_runs / cl_seg_of
in segment mode, k_cluster_big_fill and k_cluster_probe_big over several
build segments, csrc/phj_cluster.h; k_ht_fill<false>, csrc/phj_table.h; the
partitioned join over `world` segments) and the exchange block codes |
padding | bounds of every rank. A subset also runs over RCCL on a world of one
(PHJ_CTX_EXCHANGE: a padded block, segment mode, one segment).

Params are named by the form the member step takes, asserted host-only with
phj.join_path before every join (the group decides with the same radix_path):
the LDS join, the code tables, both sides fully partitioned, NoPartitioning;
one more leg reaches the code tables through PHJ_CLUSTER=0, asserted from the
result's timer names. The cases: tiny and empty relations (shards of one row
and of none), keys whose codes sit at the tables' edges (hashinv.table_edge_codes)
planted where only range sharding puts them, also under poisoned allocations
(the block's padding is never written, so it must never be read), the same
keys in every rank's shard, a cluster that is beyond the LDS limit only in the
sum over the segments (at the limit and one above it, cluster 0 and another),
runs that are mostly empty, and the world of 17 that is refused.

The expectation is always the oracle's sort-and-search count, never the
library; counts are exact. Every property a case relies on is asserted in
Python when the case is made, before the GPU is touched."""
import contextlib
import functools

import numpy as np
import pytest

import exchange_proto as X
import partitionedhashjoin_amd as phj
from hashinv import preimage
from oracle import oracle as O
from partitionedhashjoin_amd import shard_range
from test_gpu_parity import I64_MAX, I64_MIN, SEED, edge_keys
from test_gpu_preagg_resolve import CL_LIM

pytestmark = pytest.mark.gpu

MUR, XXH = phj.HASH_MURMUR3, phj.HASH_XXH3
LDS, CT, PART, NP = phj.PATH_LDS_JOIN, phj.PATH_CODE_TABLES, phj.PATH_PARTITIONED, phj.PATH_NO_PARTITIONING
PHJ_ERR_INVALID = -1   # include/phj.h

PARAMS = {   # name: (the form the member step takes, params)
    "lds-8+8-murmur3": (LDS, phj.radix_params((8, 8), hash=MUR, seed=SEED)),
    "lds-mod1024-xxh3": (LDS, phj.radix_params(num_partitions=1024, hash=XXH, seed=SEED)),
    "lds-mod1-xxh3": (LDS, phj.radix_params(num_partitions=1, hash=XXH, seed=1)),   # sub-partition bits at 40, E = 2^40
    "lds-4-xxh3": (LDS, phj.radix_params((4, 0), hash=XXH, seed=5)),                # 4 sub-partition bits
    "lds-11+11-murmur3": (LDS, phj.radix_params((11, 11), hash=MUR, seed=9)),
    "ct-8+8-murmur3": (CT, phj.radix_params((8, 8), hash=MUR, seed=SEED, stable=True)),
    "ct-mod5000-xxh3": (CT, phj.radix_params(num_partitions=5000, hash=XXH, seed=2, stable=True)),
    "ct-4-xxh3": (CT, phj.radix_params((4, 0), hash=XXH, stable=True)),
    "part-8+8-murmur3": (PART, phj.radix_params((8, 8), hash=MUR, seed=SEED, chained=True)),
    "part-mod1000-xxh3": (PART, phj.radix_params(num_partitions=1000, hash=XXH, seed=4, chained=True)),
    "np-xxh3": (NP, phj.nopart_params(hash=XXH, seed=SEED)),
    "np-murmur3-r1": (NP, phj.nopart_params(hash=MUR, seed=3, table_ratio=1.0)),
}
NAMES = list(PARAMS)
RADIX = [n for n in NAMES if PARAMS[n][0] != NP]
PER_FORM = ["lds-8+8-murmur3", "ct-8+8-murmur3", "part-8+8-murmur3", "np-xxh3"]   # one per form, one hash and seed
POISONED = PER_FORM + ["lds-mod1-xxh3", "ct-mod5000-xxh3"]
# "ct-4-xxh3": 16 partitions take one pass (no code tables) until the build side refines them into
# two (csrc/phj_capi.hip refine_plan: from |R| / 16 * 3 > 2 * 256 on)
CT_SINCE = 2731
WORLDS = (2, 3, 16)


def path(name, nR, max_s):
    """The form params `name` take over nR build rows and a largest probe
    shard of max_s rows (phj_join_path, host only), asserted to be the named one."""
    want, p = PARAMS[name]
    got = phj.join_path(p, nR, max_s)
    if want == NP:
        assert got == NP, name
    elif nR == 0:                       # no cluster plan over an empty build side
        assert got in (CT, PART), name
    elif name == "ct-4-xxh3" and nR < CT_SINCE:
        assert got == PART, (name, nR)
    else:
        assert got == want, (name, nR, max_s, got)
    return got


def shards(n, world):
    return [shard_range(n, r, world) for r in range(world)]


def max_shard(n, world):
    return max(hi - lo for lo, hi in shards(n, world))


def keys_of(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.int64).reshape(-1))


def count(R, S):
    R, S = keys_of(R), keys_of(S)
    return O.semijoin_count_keys(R, S) if len(R) and len(S) else 0


class Group:
    """One group context per world for the module, made on first use;
    fresh() closes it first (never two 16-member contexts alive) and gives a
    new one whose allocations are poisoned."""

    def __init__(self, world, flags):
        self.world, self.flags, self._c = world, flags, None

    @property
    def ctx(self):
        if self._c is None:
            self._c = phj.Context(devices=[0] * self.world, flags=self.flags)
            assert self._c.info() == (self.world, 0, self.world)
        return self._c

    def close(self):
        if self._c is not None:
            self._c.close()
            self._c = None

    @contextlib.contextmanager
    def fresh(self, poison):
        self.close()
        c = phj.Context(devices=[0] * self.world, flags=self.flags)
        try:
            c.debug_poison_alloc(poison)
            yield c
        finally:
            c.close()


@pytest.fixture(scope="module", params=WORLDS, ids=[f"w{w}" for w in WORLDS])
def group(request):
    g = Group(request.param, phj.CTX_LOCAL)
    yield g
    g.close()


@pytest.fixture(scope="module")
def rccl():
    g = Group(1, phj.CTX_EXCHANGE)
    yield g
    g.close()


def join_all(c, world, R, S, expect, names, repeats=1):
    """Upload once; every named params' join `repeats` times (a repeat reuses
    every buffer), each after the host-only assertion of its form."""
    R, S = keys_of(R), keys_of(S)
    c.upload(phj.SIDE_BUILD, O.as_relation(R))
    c.upload(phj.SIDE_PROBE, O.as_relation(S))
    for name in names:
        path(name, len(R), max_shard(len(S), world))
        for i in range(repeats):
            got = c.join(PARAMS[name][1]).matches
            assert got == expect, (name, world, i, got, expect)


# ---- a. tiny and empty: shards of one row and of none ----

TINY_R = [1, 1, 2, 0, -1, I64_MIN, I64_MAX]
TINY_S = [1, 2, 3, 0, -1, -1, I64_MIN, I64_MAX, 5, 1]
TINY = {   # case: (R, S, semi-join count)
    "adversarial": (TINY_R, TINY_S, 8),
    "one-build-row": ([I64_MIN], TINY_S, 1),
    "one-probe-row": (TINY_R, [-1], 1),
    "empty-probe": (TINY_R, [], 0),
}


def test_tiny_shapes_shard_as_the_cases_say():
    sizes = [hi - lo for lo, hi in shards(len(TINY_R), 16)]
    assert sorted(sizes) == [0] * 9 + [1] * 7                  # 9 empty R shards, 7 of one row
    for w in WORLDS:
        assert shards(1, w)[-1] == (0, 1)                        # a single row lies in the last rank
        assert max_shard(len(TINY_S), w) >= 1 and min(hi - lo for lo, hi in shards(1, w)) == 0
    assert [hi - lo for lo, hi in shards(2, 3)] == [0, 1, 1]    # n < world: empty shards on either side


def check_tiny(c, world, case):
    R, S, expect = TINY[case]
    assert count(R, S) == expect
    join_all(c, world, R, S, expect, NAMES, repeats=2)


def check_empty_build(c, world, S):
    """Radix: 0, on the code tables or partitioned form (every rank's bounds
    all 0); NoPartitioning: the reference's error."""
    join_all(c, world, [], S, 0, RADIX, repeats=2)
    for name in ("np-xxh3", "np-murmur3-r1"):
        with pytest.raises(phj.PhjError, match="numberOfObjects"):
            c.join(PARAMS[name][1])


@pytest.mark.parametrize("case", list(TINY))
def test_tiny_and_empty(group, case):
    check_tiny(group.ctx, group.world, case)


@pytest.mark.parametrize("probe", ["probe", "no-probe"])
def test_empty_build_side(group, probe):
    check_empty_build(group.ctx, group.world, TINY_S if probe == "probe" else [])


@pytest.mark.parametrize("case", ["adversarial", "empty-probe"])
def test_tiny_and_empty_rccl(rccl, case):
    check_tiny(rccl.ctx, 1, case)


def test_empty_build_side_rccl(rccl):
    check_empty_build(rccl.ctx, 1, TINY_S)


# ---- b. edge codes across the exchange ----

@functools.lru_cache(maxsize=None)
def edge_case(name):
    """pre: the keys whose codes are the tables' empty values and their bucket
    mates under the plan's hash; base: 1 .. 20003 without them; S probes every
    planted key twice, a third of base, and misses."""
    pre = edge_keys(PARAMS[name][1])
    assert len(pre) == len(np.unique(pre)) and 130 <= len(pre) <= 145   # 141 under radix bits; h % P's mates differ with P
    base = np.arange(1, 20_004, dtype=np.int64)
    base = base[~np.isin(base, pre)]
    S = np.concatenate([pre, base[::3], pre[::-1], -base[:500]])
    hits = base[::3].shape[0]
    assert count(base, S) == hits and count(pre, S) == 2 * len(pre)
    return pre, base, S, hits


def padding_everywhere(nR, world, nseg):
    """Every rank's block has padding between its codes and its bounds."""
    ce, _ = phj.exchange_layout(max_shard(nR, world), nseg)
    return all(ce - (hi - lo) > 0 for lo, hi in shards(nR, world))


def check_edge_codes(c, world, name):
    pre, base, S, hits = edge_case(name)
    one = [name]
    for w in (2, 3, 16):   # no shard fills its 64-element-padded block
        assert len(base) % (64 * w) != 0 and padding_everywhere(len(base), w, 256)
    # planted in S only: all miss (no padding word, no empty value taken for a code)
    join_all(c, world, base, S, hits, one)
    # planted in R, in the tail of the last rank's shard: all found, no walk cut short
    tail = np.concatenate([base, pre, pre[:5]])
    assert shards(len(tail), world)[-1][1] - shards(len(tail), world)[-1][0] >= len(pre) + 5
    join_all(c, world, tail, S, hits + 2 * len(pre), one)
    join_all(c, world, tail, pre, len(pre), one)   # every planted key alone
    # in the head of rank 0's shard
    head = np.concatenate([pre, base])
    assert shards(len(head), world)[0][1] >= len(pre)
    join_all(c, world, head, S, hits + 2 * len(pre), one)
    # alone: 141 rows, far shorter than the padded block (8-9 rows per shard at world 16)
    assert padding_everywhere(len(pre), world, 256)
    join_all(c, world, pre, S, 2 * len(pre), one, repeats=2)


@pytest.mark.parametrize("name", NAMES)
def test_edge_codes_across_the_exchange(group, name):
    check_edge_codes(group.ctx, group.world, name)


@pytest.mark.parametrize("name", PER_FORM + ["lds-mod1-xxh3"])
def test_edge_codes_across_the_exchange_rccl(rccl, name):
    check_edge_codes(rccl.ctx, 1, name)


def check_poisoned(g, name, poison):
    """The S-only planting on a fresh context whose every allocation is filled
    with `poison`: table_edge_codes holds 2^64 - 1 and 0, so a padding word of
    either value would be found if it were read. Nothing writes the padding
    (no memset in the timed step): after the join it still holds the poison."""
    pre, base, S, hits = edge_case(name)
    form, p = PARAMS[name]
    world = g.world
    with g.fresh(poison) as c:
        join_all(c, world, base, S, hits, [name], repeats=2)
        if form == NP:
            return
        nseg, _ = X.geometry(p, len(base))
        ce, be = phj.exchange_layout(max_shard(len(base), world), nseg)
        fill = np.frombuffer(bytes([poison]) * 8, dtype=np.int64)[0]
        for r, (lo, hi) in enumerate(shards(len(base), world)):
            blk = c.debug_exchange_block(r, be)
            assert ce > hi - lo and np.all(blk[hi - lo:ce] == fill), (name, r)
            bounds = blk[ce:].view(np.uint32)[:nseg + 1]
            assert bounds[0] == 0 and bounds[nseg] == hi - lo and np.all(np.diff(bounds.astype(np.int64)) >= 0)


@pytest.mark.parametrize("poison", [0xFF, 0x00], ids=["ff", "00"])
@pytest.mark.parametrize("name", POISONED)
def test_edge_codes_poisoned(group, name, poison):
    check_poisoned(group, name, poison)


@pytest.mark.parametrize("poison", [0xFF, 0x00], ids=["ff", "00"])
@pytest.mark.parametrize("name", PER_FORM[:2])
def test_edge_codes_poisoned_rccl(rccl, name, poison):
    check_poisoned(rccl, name, poison)


# ---- c. duplicates across segments ----

@functools.lru_cache(maxsize=None)
def dup_case():
    rng = np.random.default_rng(701)
    keys = rng.choice(np.arange(-50_000, 50_000, dtype=np.int64), 3000, replace=False)
    S = np.concatenate([keys[::2], keys[:10], keys[:10], keys[1::3] + 200_000, [I64_MIN, 0]])
    rng.shuffle(S)
    return keys, S, count(keys, S)


def check_duplicates(c, world, names):
    keys, S, expect = dup_case()
    copies = max(world, 2)
    R = np.tile(keys, copies)   # the same 3 000 keys in every rank's shard
    if world > 1:
        assert all(np.array_equal(R[lo:hi], keys) for lo, hi in shards(len(R), world))
    assert count(R, S) == expect >= 1500
    join_all(c, world, R, S, expect, names)
    # one key on both sides: every tuple in one partition, one bucket chain, every segment
    R = np.full(3000, 42, dtype=np.int64)
    S = np.concatenate([np.full(50_000, 42, dtype=np.int64), np.arange(100, dtype=np.int64)])
    assert count(R, S) == 50_001
    join_all(c, world, R, S, 50_001, names)


@pytest.mark.parametrize("name", NAMES)
def test_duplicates_across_segments(group, name):
    check_duplicates(group.ctx, group.world, [name])


def test_duplicates_across_segments_rccl(rccl):
    check_duplicates(rccl.ctx, 1, PER_FORM)


# ---- d. a cluster that is big only in the sum over the segments ----

BIG = ["lds-8+8-murmur3", "ct-8+8-murmur3", "part-8+8-murmur3"]   # one hash and seed: the same codes
HOT_CODE = {0x00: (0x1234 << 32) | 0x0042, 0x5A: (0x1234 << 32) | 0x5A42}   # cluster = bits 8..15 of 256 clusters


def big_codes(keys):
    return X.codes_of(keys, PARAMS[BIG[0]][1]).view(np.uint64)


@functools.lru_cache(maxsize=None)
def big_pool():
    """Distinct keys outside the two hot clusters; the keys of code 0 (in
    cluster 0, whose empty value is E_0 = 2^8, not 0) and of E_0 itself."""
    rng = np.random.default_rng(401)
    pool = np.unique(rng.integers(-(1 << 40), 1 << 40, 240_000, dtype=np.int64))
    rng.shuffle(pool)
    cl = (big_codes(pool) >> np.uint64(8)) & np.uint64(0xFF)
    pool = pool[~np.isin(cl, np.array(list(HOT_CODE), dtype=np.uint64))]
    key0, keyE = preimage(True, 0, SEED), preimage(True, 1 << 8, SEED)
    assert list(big_codes([key0, keyE])) == [0, 1 << 8] and len(pool) > 16 * (CL_LIM + 65) + 3000
    return pool, key0, keyE


@functools.lru_cache(maxsize=4)
def big_case(world, k, placement, cluster, with0):
    """k copies of one hot key among other clusters' keys: interleaved, every
    rank holds about k / world of them (20 000 others); or all of them in the
    last rank's shard (as many others as make that shard k + 64 rows). The key
    of code 0 stands in rank 0's shard or nowhere."""
    p = PARAMS[BIG[0]][1]
    pool, key0, keyE = big_pool()
    hot = preimage(True, HOT_CODE[cluster], SEED)
    assert int(big_codes([hot])[0]) == HOT_CODE[cluster] and k in (CL_LIM, CL_LIM + 1)
    if placement == "interleaved":
        n = 20_000 + k
        at = (np.arange(k, dtype=np.int64) * n) // k
    else:
        n = world * (k + 64)
        at = np.arange(n - (k + 64), n - 64, dtype=np.int64)
    mask = np.zeros(n, dtype=bool)
    mask[at] = True
    assert int(mask.sum()) == k
    R = np.empty(n, dtype=np.int64)
    R[mask] = hot
    others = pool[:n - k].copy()
    if with0:
        others[0] = key0
    R[~mask] = others
    nseg, segment_of = X.geometry(p, n)
    assert nseg == 256 and phj.exchange_geometry(p, n)[4]            # 256 clusters at every size here
    seg = segment_of(X.codes_of(R, p))
    assert int((seg == cluster).sum()) == k + (1 if with0 and cluster == 0 else 0)
    per = [int((seg[lo:hi] == cluster).sum()) for lo, hi in shards(n, world)]
    if placement == "interleaved" and world > 1:
        assert max(per) < CL_LIM and min(per) >= k // world - 1       # no segment's run is big by itself
    elif world > 1:
        assert per[-1] == k and sum(per[1:-1]) == 0 and mask[shards(n, world)[-1][0]:].sum() == k
    hits = others[1::7][:4000]
    S = np.concatenate([np.full(50, hot, dtype=np.int64), [key0, keyE], hits, pool[n - k:n - k + 3000]])
    np.random.default_rng(k + cluster).shuffle(S)
    expect = 50 + (1 if with0 else 0) + len(hits)
    assert count(R, S) == expect
    return R, S, expect


def check_big(c, world, k, placement, cluster):
    for with0 in (True, False):
        R, S, expect = big_case(world, k, placement, cluster, with0)
        join_all(c, world, R, S, expect, BIG)


@pytest.mark.parametrize("cluster", [0x00, 0x5A], ids=["cluster0", "cluster5a"])
@pytest.mark.parametrize("placement", ["interleaved", "one-rank"])
@pytest.mark.parametrize("k", [CL_LIM, CL_LIM + 1], ids=["at-limit", "above-limit"])
def test_big_cluster_over_segments(group, k, placement, cluster):
    check_big(group.ctx, group.world, k, placement, cluster)


@pytest.mark.parametrize("k", [CL_LIM, CL_LIM + 1], ids=["at-limit", "above-limit"])
def test_big_cluster_rccl(rccl, k):
    check_big(rccl.ctx, 1, k, "interleaved", 0x00)


# ---- e. sparse runs: most (cluster, rank) runs empty, or none ----

@functools.lru_cache(maxsize=None)
def sparse_case(nR):
    rng = np.random.default_rng(nR)
    R = rng.choice(np.arange(-2_000_000, 2_000_000, dtype=np.int64), nR, replace=False)
    S = np.concatenate([rng.choice(R, nR), rng.integers(3_000_000, 9_000_000, nR + 1, dtype=np.int64)])   # half misses
    rng.shuffle(S)
    assert count(R, S) == nR          # the misses lie outside R's key range
    return R, S, nR


@pytest.mark.parametrize("nR", [1000, 200_003])
def test_sparse_and_full_runs(group, nR):
    R, S, expect = sparse_case(nR)
    p = PARAMS["lds-8+8-murmur3"][1]
    nseg, segment_of = X.geometry(p, nR)
    runs = [np.bincount(segment_of(X.codes_of(R[lo:hi], p)), minlength=nseg) for lo, hi in shards(nR, group.world)]
    if nR == 1000 and group.world == 16:
        assert nseg * group.world > 4 * nR                      # over three quarters of the runs are empty
        assert max(int((np.stack(runs)[:, d] > 0).sum()) for d in range(nseg)) < 16
    if nR == 200_003:
        assert all(int(r.min()) > 0 for r in runs)              # no run is empty
    join_all(group.ctx, group.world, R, S, expect, NAMES)


def test_sparse_runs_rccl(rccl):
    R, S, expect = sparse_case(1000)
    join_all(rccl.ctx, 1, R, S, expect, PER_FORM)


# ---- the code tables through the tuning knob ----

def timer_names(r):
    return {t for t, _, _ in r.timers()}


def assert_code_table_form(r, what):
    """csrc/phj_group.h member_radix: the code-table form times `build`
    (build_ht) and `probe` (probe_ht) behind `exchange`; only the LDS join
    lists build.big, only the partitioned form gives S a pass 2."""
    names = timer_names(r)
    assert {"exchange", "build", "probe"} <= names and "build.big" not in names, (what, names)
    assert not [n for n in names if n.startswith("S.p2")], (what, names)


def test_code_tables_by_tuning_knob(monkeypatch, group):
    """PHJ_CLUSTER=0 (read when the context is created): plain (8,8) and
    -p 1024 take the unordered pass 1 and the code tables over `world`
    segments. phj_join_path knows only default tuning, so the form is read
    from the timers; -p 1024 refines to two passes (and code tables) from
    about 175K build rows on."""
    monkeypatch.setenv("PHJ_CLUSTER", "0")
    world = group.world
    group.close()   # (never two 16-member contexts alive)
    with phj.Context(devices=[0] * world, flags=phj.CTX_LOCAL) as c:
        def run(name, R, S, expect):
            c.upload(phj.SIDE_BUILD, O.as_relation(keys_of(R)))
            c.upload(phj.SIDE_PROBE, O.as_relation(keys_of(S)))
            for _ in range(2):
                r = c.join(PARAMS[name][1])
                assert r.matches == expect, (name, world)
                assert_code_table_form(r, name)
        name = "lds-8+8-murmur3"
        pre, base, S, hits = edge_case(name)
        run(name, base, S, hits)
        run(name, np.concatenate([pre, base, pre]), S, hits + 2 * len(pre))
        run(name, pre, S, 2 * len(pre))
        run(name, *big_case(world, CL_LIM + 1, "interleaved", 0x00, True))   # a partition beyond k_ht_fill's LDS slice
        run(name, *sparse_case(1000))
        name = "lds-mod1024-xxh3"
        pre, _, _, _ = edge_case(name)
        R, S, _ = sparse_case(200_003)
        R, S = np.concatenate([R, pre]), np.concatenate([pre[::-1], S, pre])
        run(name, R, S, count(R, S))
        run(name, R[:-len(pre)], S, count(R[:-len(pre)], S))


# ---- f. more ranks than build segments ----

def test_world_of_17_is_refused():
    """kMaxSegs = 16 build segments: phj_ctx_create_ex and phj_ctx_create_rank
    refuse a larger world with PHJ_ERR_INVALID before any member is created
    (include/phj.h), so group_join's own PHJ_ERR_RANGE is never reached."""
    with pytest.raises(phj.PhjError) as e:
        phj.Context(devices=[0] * 17, flags=phj.CTX_LOCAL)
    assert e.value.code == PHJ_ERR_INVALID
    with pytest.raises(phj.PhjError) as e:
        phj.Context.rank(0, 17, 0, bytes(128))
    assert e.value.code == PHJ_ERR_INVALID
