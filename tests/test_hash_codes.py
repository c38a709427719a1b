"""Hash codes stand in for keys in the counting join (csrc/phj_hash.h kHashed).

The keys-only pass 1 writes h(k) instead of k and the code tables store h(r),
so the probe compares codes. That counts the key matches of
/root/reference/src/RadixCluster/HashJoin.hpp:295-301 exactly iff h is a
bijection of the 64-bit keys. Here both hashes are inverted step by step
(against the oracle's forward hashes, which are pinned to xxhash / the
canonical fmix64 constants) on random and extreme keys and several seeds:
a left inverse on every sample is that bijection, observed.

The same inverses craft the keys of tests/test_gpu_collisions.py
(hashinv.partition_mates, hashinv.np_edge_keys); where those keys go, their
partition, LDS bucket and NoPartitioning home bucket, is restated in numpy
from the kernels' formulas and asserted here, without a GPU.
"""
import numpy as np
import pytest

from oracle import oracle as O
from hashinv import (lds_bucket, murmur3_inverse, np_edge_keys, np_geometry, np_home, odd_part, partition_mates,
                     partition_of, preimage, table_edge_codes, xxh3_inverse)

M64 = (1 << 64) - 1
SEEDS = [0, 1, 0x0BAD_5EED_0BAD_5EED, 0xFFFF_FFFF_FFFF_FFFF]


def _keys():
    rng = np.random.default_rng(7)
    k = [0, 1, 2, -1, 2**63 - 1, -(2**63), 2**32, 2**32 - 1, -(2**32), 10_000_000]
    k += [int(v) for v in rng.integers(-(2**63), 2**63 - 1, 150, dtype=np.int64)]
    k += list(range(1, 40))
    return k


@pytest.mark.parametrize("seed", SEEDS)
def test_murmur3_is_a_bijection(seed):
    for k in _keys():
        u = k & M64
        h = O.murmur3(u, seed) & M64
        assert murmur3_inverse(h, seed) == u


@pytest.mark.parametrize("seed", SEEDS)
def test_xxh3_is_a_bijection(seed):
    for k in _keys()[:60]:
        u = k & M64
        h = O.xxh3(u, seed) & M64
        assert xxh3_inverse(h, seed) == u


def test_codes_preserve_the_join_count():
    # counting over codes == counting over keys, for both hashes
    rng = np.random.default_rng(3)
    r = rng.integers(-5000, 5000, 3000, dtype=np.int64)
    s = rng.integers(-9000, 9000, 20000, dtype=np.int64)
    s[::5] = r[: len(s[::5]) % len(r) or 1][0]
    expect = O.semijoin_count_keys(r, s)
    for kind in (O.HASH_MURMUR3, O.HASH_XXH3):
        hr = O.hash_keys(kind, r, 11).view(np.int64)
        hs = O.hash_keys(kind, s, 11).view(np.int64)
        assert O.semijoin_count_keys(hr, hs) == expect


@pytest.mark.parametrize("nparts", [0, 1, 32, 1000, 5000])
def test_edge_code_preimages(nparts):
    # the keys the GPU parity tests plant (test_gpu_parity.py
    # test_empty_value_preimages): each hashes to its chosen code
    codes = table_edge_codes(nparts)
    assert {0, 1, 1 << 40} <= set(codes)
    for kind, mur in ((O.HASH_MURMUR3, True), (O.HASH_XXH3, False)):
        for seed in (1, 0x1234_5678_9ABC_DEF1):
            keys = np.array([preimage(mur, c, seed) for c in codes], dtype=np.int64)
            assert np.array_equal(O.hash_keys(kind, keys, seed), np.array(codes, dtype=np.uint64))


def test_known_code_one_key():
    # under XXH3 seed 1 this key's code is 1, which the
    # round-3 tables used as partition 0's empty value under h % 1
    k = -6993838658721465140
    assert preimage(False, 1, 1) == k
    assert int(O.hash_keys(O.HASH_XXH3, np.array([k], dtype=np.int64), 1)[0]) == 1


def _crafting_params():
    # the plans the row-join tests run (test_gpu_materialize.PARAMS): both
    # hashes with the seeds used there
    from test_gpu_materialize import PARAMS
    return PARAMS


@pytest.mark.parametrize("name", ["radix-8+8", "radix-mod1024", "radix-4"])
def test_partition_mates_share_partition_and_bucket(name):
    params = {p[0]: p[1] for p in _crafting_params()}[name]
    m = odd_part(params.num_partitions)
    assert m == 1   # 1024 = 2^10: the three plans allow 2^14 mates
    for base in (0, 12345, (1 << 50) - 1):
        keys = partition_mates(params, 700, base)
        assert len(np.unique(keys)) == 700
        h = O.hash_keys(params.hash, keys, params.hash_seed)
        assert np.array_equal(h, np.uint64(base) + (np.arange(700, dtype=np.uint64) << np.uint64(50)))
        # one partition under the requested plan and under every refinement
        # that stays within 2^22 partitions (h % P: ten bits from bit 40 on)
        logp = 10 if params.num_partitions else int(params.radix_bits[0]) + int(params.radix_bits[1])
        for s in range(0, (10 if params.num_partitions else 22 - logp) + 1):
            q = partition_of(h, params, s)
            assert np.all(q == q[0])
        assert int(partition_of(h, params)[0]) == (base % 1024 if params.num_partitions else base & ((1 << logp) - 1))
        # one LDS bucket at every round size (bucket_of: (h >> 32) & (nbk - 1), nbk <= 128)
        assert np.all((h >> np.uint64(32)) & np.uint64(127) == np.uint64((base >> 32) & 127))
        for nbk in (1, 2, 64, 128):
            assert len(np.unique(lds_bucket(h, nbk))) == 1


def test_partition_mates_odd_partition_counts():
    # h % P with odd factors: L = 2^50 odd(P) keeps the residue, and the
    # helper refuses more mates than fit below 2^64
    from partitionedhashjoin_amd import radix_params
    for P, mur, seed in ((1000, True, 3), (5000, False, 7), (3, False, 1), (1 << 22, True, 2)):
        params = radix_params(num_partitions=P, hash=O.HASH_MURMUR3 if mur else O.HASH_XXH3, seed=seed)
        m = odd_part(P)
        assert P % m == 0 and m % 2 == 1 and (P // m) & (P // m - 1) == 0
        most = ((1 << 14) - 1) // m + 1
        keys = partition_mates(params, most, 77)
        h = O.hash_keys(params.hash, keys, seed)
        assert len(np.unique(keys)) == most
        assert np.all(h % np.uint64(P) == np.uint64(77 % P))
        assert len(np.unique(lds_bucket(h))) == 1
        with pytest.raises(ValueError):
            partition_mates(params, most + 1, 77)
    with pytest.raises(ValueError):
        partition_mates(params, 2, 1 << 50)


def test_np_geometry_restates_the_build():
    # csrc/phj_capi.hip np_build by hand: 380 tuples at 2 slots each are 109
    # buckets, one region's worth, but two regions are the minimum: 2 x 55
    assert np_geometry(380, 0.0) == (110, 55, 1)
    assert np_geometry(380, 1.0) == (56, 28, 1)
    assert np_geometry(1400, 1.0) == (200, 100, 1)    # 7 x 200 slots: exactly full
    assert np_geometry(10_000_000, 0.0) == (4096 * 698, 698, 12)
    assert np_geometry(1, 1.0) == (2, 1, 1)


@pytest.mark.parametrize("name", ["np-xxh3", "np-murmur-r1"])
def test_np_edge_keys_home_buckets(name):
    params = {p[0]: p[1] for p in _crafting_params()}[name]
    geoms = [np_geometry(n, r) for n in (380, 1400, 50_000, 10_000_000) for r in (1.0, 0.0)]
    geoms += [(3 << 22, 3, 22), (2 * 1024, 1024, 1)]
    assert len({g[2] for g in geoms}) >= 4
    want = {"last_of_table": lambda nb, nbr: nb - 1, "last_of_region0": lambda nb, nbr: nbr - 1,
            "first_of_table": lambda nb, nbr: 0, "first_of_region1": lambda nb, nbr: nbr}
    seen = []
    for where, home in want.items():
        keys = np_edge_keys(params, where, 1024)
        assert len(np.unique(keys)) == 1024
        seen.append(keys)
        h = O.hash_keys(params.hash, keys, params.hash_seed)
        for nb, nbr, rbits in geoms:
            assert 1 <= rbits <= 22 and nb == nbr << rbits
            # np_home_r written out: region r = h & (2^rbits - 1), bucket r nbr + ((h >> 32) nbr >> 32)
            r = h & np.uint64((1 << rbits) - 1)
            b = r * np.uint64(nbr) + (((h >> np.uint64(32)) * np.uint64(nbr)) >> np.uint64(32))
            assert np.array_equal(b, np_home(h, (nb, nbr, rbits)))
            assert np.all(b == np.uint64(home(nb, nbr))), (where, nb, nbr, rbits)
    # first_of_table and last_of_region0 share their low bits only: all four sets are disjoint
    assert len(np.unique(np.concatenate(seen))) == 4 * 1024
    with pytest.raises(ValueError):
        np_edge_keys(params, "last_of_table", 1025)
