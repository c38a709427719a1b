"""Ordinals on the retained key index (phj_index_build_ex with
PHJ_INDEX_ORDINALS; phj_index_uniques / _encode / _accumulate) on the GPU. The
expectation is always numpy, never the library: np.unique(return_index=True),
ordinals = the rank of the first rows, np.bincount for counts, np.add.at on
uint64 for sums. Every output is a preallocated device buffer between 0xA5
canaries (test_gpu_index.DevOut)."""
import ctypes as C
import functools

import numpy as np
import pytest

import partitionedhashjoin_amd as phj
from partitionedhashjoin_amd import _capi
from hashinv import NP_EDGES, np_edge_keys
from oracle import oracle as O
from test_gpu_index import (DevOut, Job, HASHES, HASH_IDS, SPECIAL, basic_case, dev_keys, expected, keys_of_fast,
                            lookup, params_of, tuples)

pytestmark = pytest.mark.gpu
R_, S_ = phj.SIDE_BUILD, phj.SIDE_PROBE


def ordinals_of(Rk):
    """(sorted distinct keys, their ordinals, first_rows): the ordinal of a key
    is the rank of its first row among the distinct keys' first rows."""
    Rk = np.asarray(Rk, dtype=np.int64)
    u, first = np.unique(Rk, return_index=True)
    order = np.argsort(first, kind="stable")
    rank = np.empty(len(u), dtype=np.int64)
    rank[order] = np.arange(len(u))
    return u, rank, first[order].astype(np.int64)


def expected_codes(Rk, Sk):
    Sk = np.asarray(Sk, dtype=np.int64)
    u, rank, _ = ordinals_of(Rk)
    if len(u) == 0:
        return np.full(len(Sk), -1, dtype=np.int64)
    pos = np.minimum(np.searchsorted(u, Sk), len(u) - 1)
    return np.where(u[pos] == Sk, rank[pos], -1).astype(np.int64)


def expected_groups(Rk, Sk, values=None):
    """(counts uint64, sums uint64 modulo 2^64, missing) by bincount / add.at."""
    codes = expected_codes(Rk, Sk)
    d = len(np.unique(np.asarray(Rk, dtype=np.int64)))
    hit = codes >= 0
    counts = np.bincount(codes[hit], minlength=d).astype(np.uint64)
    sums = np.zeros(d, dtype=np.uint64)
    if values is not None:
        np.add.at(sums, codes[hit], np.asarray(values, dtype=np.int64)[hit].view(np.uint64))
    return counts, sums, int((~hit).sum())


class EncJob(Job):
    def enqueue(self, ix):
        ix.encode(self.keys, self.n, self.rows.ptr, self.found.ptr, self.count.ptr, key_stride=self.stride)


class Acc:
    """Zeroed, guarded accumulators of d groups and a missing counter."""

    def __init__(self, slot, d, sums=True):
        self.d = d
        self.counts = DevOut(slot + ".n", 8 * d, fill=0)
        self.sums = DevOut(slot + ".s", 8 * d, fill=0) if sums else None
        self.missing = DevOut(slot + ".m", 8, fill=0)

    def add(self, ix, slot, Sk, values=None, stride=1, vstride=1):
        """Enqueue one batch (its inputs are copied to the device first)."""
        Sk = np.asarray(Sk, dtype=np.int64)
        src = Sk if stride == 1 else np.stack([Sk, np.roll(Sk, 1)], axis=1).reshape(-1)
        kp = dev_keys(slot + ".k", src)
        vp = None
        if values is not None:
            values = np.asarray(values, dtype=np.int64)
            vsrc = values if vstride == 1 else np.stack([values, ~values], axis=1).reshape(-1)
            vp = dev_keys(slot + ".v", vsrc)
        ix.accumulate(kp, len(Sk), self.counts.ptr, vp, self.sums.ptr if values is not None else None, self.missing.ptr,
                      key_stride=stride, value_stride=vstride)

    def results(self):
        sums = self.sums.read().view(np.uint64) if self.sums is not None else None
        return self.counts.read().view(np.uint64), sums, int(self.missing.read().view(np.uint64)[0])


def encode(ctx, ix, Sk, stride=1, found_off=0, slot="a"):
    j = EncJob(slot, Sk, stride, found_off)
    j.enqueue(ix)
    ctx.synchronize()
    codes, found = j.results()
    return codes, found, int(j.count.read().view(np.uint64)[0])


def check_encode(ctx, ix, Rk, Sk, **kw):
    exp = expected_codes(Rk, Sk)
    codes, found, cnt = encode(ctx, ix, Sk, **kw)
    bad = np.flatnonzero(codes != exp)
    assert len(bad) == 0, (len(bad), bad[:5], codes[bad[:5]], exp[bad[:5]])
    assert set(np.unique(found)) <= {0, 1} and np.array_equal(found.astype(bool), exp >= 0)
    assert cnt == int((exp >= 0).sum())
    return exp


def check_index(ctx, ix, Rk):
    """first_rows, the distinct count, and factorize of the build column itself."""
    Rk = np.asarray(Rk, dtype=np.int64)
    u, rank, first_rows = ordinals_of(Rk)
    assert ix.ordinals
    info = ix.info()
    assert info.distinct == len(u) == ix.result.matches
    ptr, n = ix.first_rows_ptr()
    assert n == len(u) and (ptr % 8 == 0) and (ptr != 0) == (n > 0)
    got = ix.first_rows()
    assert np.array_equal(got, first_rows)
    assert info.table_bytes == info.nb * 64 + 8 * len(u)
    if len(Rk):
        codes = check_encode(ctx, ix, Rk, Rk, slot="self")
        assert np.array_equal(Rk[got][codes], Rk)
    return first_rows


def check_acc(ctx, ix, Rk, Sk, values=None, stride=1, vstride=1, slot="acc"):
    d = len(np.unique(np.asarray(Rk, dtype=np.int64)))
    acc = Acc(slot, d, sums=values is not None)
    acc.add(ix, slot, Sk, values, stride, vstride)
    ctx.synchronize()
    counts, sums, missing = acc.results()
    ec, es, em = expected_groups(Rk, Sk, values)
    assert np.array_equal(counts, ec), np.flatnonzero(counts != ec)[:5]
    if values is not None:
        assert np.array_equal(sums, es), np.flatnonzero(sums != es)[:5]
    assert missing == em


def bind(ctx, binding, Rk):
    Rk = np.asarray(Rk, dtype=np.int64)
    if binding == "tuples":
        ctx.upload(R_, tuples(Rk, 1000))
    elif binding == "columns":
        ctx.upload_columns(R_, Rk, np.arange(len(Rk), dtype=np.int64))
    else:
        ctx.upload_columns(R_, Rk)


# ---- 1. basic ----

@pytest.mark.parametrize("binding", ["tuples", "columns", "keys"])
@pytest.mark.parametrize("name,hash_", HASHES, ids=HASH_IDS)
def test_ordinal_basic(ctx, name, hash_, binding):
    Rk, Sk = basic_case()
    bind(ctx, binding, Rk)
    p = params_of(hash_)
    with ctx.build_index(p, ordinals=True) as ix:
        names = [t[0] for t in ix.result.timers()]
        assert "index.ordinals" in names and "index.build" in names
        check_index(ctx, ix, Rk)
        for stride in (1, 2):
            for off in (0, 1):
                exp = check_encode(ctx, ix, Rk, Sk, stride=stride, found_off=off)
        assert 0.25 < (exp < 0).mean() < 0.45
        codes, found = ix.encode_host(Sk[:1000])
        assert found.dtype == bool and np.array_equal(codes, exp[:1000]) and np.array_equal(found, exp[:1000] >= 0)
        rows_ord = lookup(ctx, ix, Sk)
        with ctx.build_index(p) as plain:
            assert not plain.ordinals
            assert "index.ordinals" not in [t[0] for t in plain.result.timers()]
            rows_plain = lookup(ctx, plain, Sk)
        assert np.array_equal(rows_ord[0], expected(Rk, Sk))
        assert np.array_equal(rows_ord[0], rows_plain[0]) and np.array_equal(rows_ord[1], rows_plain[1])
        assert rows_ord[2] == rows_plain[2]
        rows2, _, _ = lookup(ctx, ix, Sk[:20_001], stride=2, found_off=3)
        assert np.array_equal(rows2, expected(Rk, Sk[:20_001]))


# ---- 2. word and scan edges ----

EDGE_ROWS = [0, 1, 31, 32, 33, 4095, 4096, 4097, 131071, 131072, 131073, 262145]


def edge_pattern(pattern, n):
    """distinct: a shuffled run of distinct keys. equal: one key. twice: every
    key twice, one copy in each half of the rows (the copies of the second half
    shuffled; with an odd n the last row's key occurs once, so its first
    occurrence lies in the second half)."""
    rng = np.random.default_rng(1000 + n)
    if pattern == "distinct":
        return rng.permutation(n).astype(np.int64) * 5 - 7
    if pattern == "equal":
        return np.full(n, 424_242, dtype=np.int64)
    h = n // 2
    half = rng.permutation(h).astype(np.int64) * 3 + 11
    return np.concatenate([half, rng.permutation(half), np.full(n - 2 * h, -5, dtype=np.int64)])


@pytest.mark.parametrize("pattern", ["distinct", "equal", "twice"])
@pytest.mark.parametrize("name,hash_", HASHES, ids=HASH_IDS)
def test_ordinal_word_and_scan_edges(ctx, name, hash_, pattern):
    p = params_of(hash_)
    for n in EDGE_ROWS:
        Rk = edge_pattern(pattern, n)
        ctx.upload_columns(R_, Rk)
        with ctx.build_index(p, ordinals=True) as ix:
            first = check_index(ctx, ix, Rk)
            if pattern == "distinct":
                assert np.array_equal(first, np.arange(n))
            elif pattern == "equal":
                assert len(first) == min(n, 1)
            else:
                assert np.array_equal(first[:n // 2], np.arange(n // 2)) and len(first) == n // 2 + n % 2
            check_encode(ctx, ix, Rk, [1, -5, 424_242, 2, 11, 12], slot="few")


# ---- 3. special keys ----

@pytest.mark.parametrize("name,hash_", HASHES, ids=HASH_IDS)
def test_ordinal_special_keys_present_and_absent(ctx, name, hash_):
    p = params_of(hash_)
    special = np.array(SPECIAL, dtype=np.int64)
    rng = np.random.default_rng(9)
    filler = np.setdiff1d(rng.integers(-2**62, 2**62, 700), special)[:600]
    rng.shuffle(filler)
    Rk = np.concatenate([filler[:100], special, filler[100:], special[::-1]])
    Sk = np.concatenate([special, filler[:50], special])
    ctx.upload_columns(R_, Rk)
    with ctx.build_index(p, ordinals=True) as ix:
        check_index(ctx, ix, Rk)
        exp = check_encode(ctx, ix, Rk, Sk)
        assert np.array_equal(exp[:4], 100 + np.arange(4))
        check_acc(ctx, ix, Rk, Sk, values=np.arange(len(Sk)) - 7)
    ctx.upload_columns(R_, filler)
    with ctx.build_index(p, ordinals=True) as ix:
        exp = check_encode(ctx, ix, filler, Sk)
        assert (exp[:4] == -1).all() and (exp[4:54] >= 0).all()
        check_acc(ctx, ix, filler, Sk, values=np.arange(len(Sk)) - 7)


# ---- 4. crafted collisions ----

def with_repeats(rng, Rk, k):
    """Rk with k of its keys appended again and everything shuffled: a key's
    lowest row may reach the table through the region build or the overflow
    pass, whichever its other rows took."""
    out = np.concatenate([Rk, rng.choice(Rk, k)])
    rng.shuffle(out)
    return out


@pytest.mark.parametrize("where", list(NP_EDGES))
@pytest.mark.parametrize("name,hash_", HASHES, ids=HASH_IDS)
def test_ordinal_crafted_edge_buckets(ctx, name, hash_, where):
    p = params_of(hash_)
    rng = np.random.default_rng(12)
    mates = np_edge_keys(p, where, 1024)
    rnd = np.setdiff1d(rng.integers(1, 2**40, 5_200), mates)[:5_000]
    Rk = with_repeats(rng, np.concatenate([rnd, mates]), 3_000)
    ctx.upload_columns(R_, Rk)
    with ctx.build_index(p, ordinals=True) as ix:
        check_index(ctx, ix, Rk)
        Sk = np.concatenate([Rk, rng.integers(2**41, 2**42, 2_000)])
        rng.shuffle(Sk)
        check_encode(ctx, ix, Rk, Sk)
        check_acc(ctx, ix, Rk, Sk, values=Sk ^ 0x55)


@pytest.mark.parametrize("name,hash_", HASHES, ids=HASH_IDS)
def test_ordinal_one_region_far_beyond_its_share(ctx, name, hash_):
    p = params_of(hash_)
    rng = np.random.default_rng(13)
    crowd = keys_of_fast(ctx, p, [(((t * 0x9E3779B1) & 0xFFFFFFFF) << 32) for t in range(20_000)])
    rnd = np.setdiff1d(rng.integers(1, 2**40, 2_100), crowd)[:2_000]
    Rk = with_repeats(rng, np.concatenate([crowd, rnd]), 10_000)
    ctx.upload_columns(R_, Rk)
    with ctx.build_index(p, ordinals=True) as ix:
        info = ix.info()
        assert info.distinct == 22_000 and info.nbr * info.slots < 20_000   # the overflow pass claimed entries
        check_index(ctx, ix, Rk)
        Sk = np.concatenate([Rk, rng.integers(2**41, 2**42, 5_000)])
        rng.shuffle(Sk)
        check_encode(ctx, ix, Rk, Sk)
        check_acc(ctx, ix, Rk, Sk, values=Sk)
        assert np.array_equal(lookup(ctx, ix, Sk)[0], expected(Rk, Sk))


# ---- 5. poison ----

@pytest.mark.parametrize("name,hash_", HASHES, ids=HASH_IDS)
def test_ordinal_poisoned_workspace(name, hash_):
    Rk, Sk = basic_case()
    with phj.Context(0) as c:
        c.debug_poison_alloc(0xFF)
        c.upload(R_, tuples(Rk))
        with c.build_index(params_of(hash_), ordinals=True) as ix:
            check_index(c, ix, Rk)
            check_encode(c, ix, Rk, Sk, slot="poison")
            check_acc(c, ix, Rk, Sk, values=Sk * 3, slot="poison")


# ---- 6. in-stream ----

@pytest.mark.parametrize("name,hash_", HASHES, ids=HASH_IDS)
def test_ordinal_calls_are_enqueued_and_the_index_is_retained(ctx, name, hash_):
    Rk, Sk = basic_case()
    rng = np.random.default_rng(21)
    R2 = rng.integers(1_000, 4_000, 2_500)
    vals = rng.integers(-2**40, 2**40, len(Sk))
    p = params_of(hash_)
    ctx.upload(R_, tuples(Rk))
    ctx.upload(S_, tuples(Sk))
    d = len(np.unique(Rk))
    cuts = [0, 5_001, 33_333, 50_000]
    with ctx.build_index(p, ordinals=True) as ix:
        shared = DevOut("enq.count", 8, fill=0)
        jobs = [EncJob(f"enq{i}", Sk[cuts[i]:cuts[i + 1]], found_off=i, count=shared) for i in range(3)]
        acc = Acc("enq.acc", d)
        kp = [dev_keys(f"enq.k{i}", Sk[i::2]) for i in range(2)]
        vp = [dev_keys(f"enq.v{i}", vals[i::2]) for i in range(2)]
        for j in jobs:              # back to back, no call in between
            j.enqueue(ix)
        for i in range(2):
            ix.accumulate(kp[i], len(Sk[i::2]), acc.counts.ptr, vp[i], acc.sums.ptr, acc.missing.ptr)
        ctx.synchronize()
        total = 0
        for i, j in enumerate(jobs):
            exp = expected_codes(Rk, Sk[cuts[i]:cuts[i + 1]])
            codes, found = j.results()
            assert np.array_equal(codes, exp) and np.array_equal(found.astype(bool), exp >= 0)
            total += int((exp >= 0).sum())
        assert int(shared.read().view(np.uint64)[0]) == total
        counts, sums, missing = acc.results()
        ec, es, em = expected_groups(Rk, Sk, vals)
        assert np.array_equal(counts, ec) and np.array_equal(sums, es) and missing == em
        # a join, a rebind and a second (plain) index on the same context
        assert ctx.join(p).matches == int(np.isin(Sk, Rk).sum())
        ctx.upload(R_, tuples(R2))
        assert ctx.join(p).matches == int(np.isin(Sk, R2).sum())
        with ctx.build_index(p) as plain:
            assert np.array_equal(lookup(ctx, plain, Sk)[0], expected(R2, Sk))
            check_encode(ctx, ix, Rk, Sk)
        check_index(ctx, ix, Rk)
        check_acc(ctx, ix, Rk, Sk, values=vals)


# ---- 7. wrong state ----

def test_ordinal_wrong_state(ctx):
    Rk, Sk = basic_case()
    ctx.upload(R_, tuples(Rk))
    keys = dev_keys("err.k", Sk[:100])
    out = DevOut("err.r", 8 * 100)
    acc = DevOut("err.a", 8 * 2_000)
    p = params_of(phj.HASH_XXH3)
    L = ctx._L

    def raw_calls(c, h):
        ptr, n = C.c_void_p(), C.c_uint64(0)
        return [L.phj_index_encode(c._h, h, C.c_void_p(keys), 1, 100, C.c_void_p(out.ptr), None, None),
                L.phj_index_uniques(c._h, h, C.byref(ptr), C.byref(n)),
                L.phj_index_accumulate(c._h, h, C.c_void_p(keys), 1, None, 1, 100, C.c_void_p(acc.ptr), None, None)]

    with ctx.build_index(p) as plain:
        assert not plain.ordinals
        assert raw_calls(ctx, plain._h) == [_capi.PHJ_ERR_STATE] * 3
        with pytest.raises(phj.PhjError, match="without ordinals") as e:
            plain.encode(keys, 100, out.ptr)
        assert e.value.code == _capi.PHJ_ERR_STATE
        for call in (plain.first_rows, lambda: plain.accumulate(keys, 100, acc.ptr)):
            with pytest.raises(phj.PhjError, match="without ordinals"):
                call()
    with ctx.build_index(p, ordinals=True) as ix:
        with phj.Context(0) as other:           # an index belongs to its context
            assert raw_calls(other, ix._h) == [_capi.PHJ_ERR_INVALID] * 3
        with pytest.raises(phj.PhjError) as e:    # sums without values, values without sums
            ix.accumulate(keys, 100, acc.ptr, None, acc.ptr)
        assert e.value.code == _capi.PHJ_ERR_INVALID
        with pytest.raises(phj.PhjError) as e:
            ix.accumulate(keys, 100, acc.ptr, keys, None)
        assert e.value.code == _capi.PHJ_ERR_INVALID
        for kw in (dict(key_stride=3), dict(value_stride=0)):
            with pytest.raises(phj.PhjError) as e:
                ix.accumulate(keys, 100, acc.ptr, keys, acc.ptr + 8_000, **kw)
            assert e.value.code == _capi.PHJ_ERR_INVALID
        with pytest.raises(phj.PhjError) as e:
            ix.accumulate(keys, 100, None)
        assert e.value.code == _capi.PHJ_ERR_INVALID
        ix.accumulate(None, 0, None)            # n == 0: nothing is launched or written
        ix.encode(None, 0, None)
        assert L.phj_index_build_ex(None, C.byref(p), 1, None, None) == _capi.PHJ_ERR_INVALID
    h, r = C.c_void_p(), phj.JoinResult()
    assert L.phj_index_build_ex(ctx._h, C.byref(p), 2, C.byref(h), C.byref(r)) == _capi.PHJ_ERR_INVALID
    assert not h.value
    assert L.phj_index_build_ex(ctx._h, C.byref(p), 3, C.byref(h), C.byref(r)) == _capi.PHJ_ERR_INVALID
    ctx.synchronize()
    assert (out.read() == 0xEE).all() and (acc.read() == 0xEE).all()


def test_ordinal_over_an_empty_build_side(ctx):
    _, Sk = basic_case()
    ctx.upload_columns(R_, np.zeros(0, dtype=np.int64))
    with ctx.build_index(params_of(phj.HASH_XXH3), ordinals=True) as ix:
        assert ix.first_rows_ptr() == (0, 0) and len(ix.first_rows()) == 0 and ix.info().distinct == 0
        exp = check_encode(ctx, ix, [], np.concatenate([Sk[:3_000], np.array(SPECIAL, dtype=np.int64)]))
        assert (exp == -1).all()
        check_acc(ctx, ix, [], Sk[:3_000], values=Sk[:3_000])


# ---- 8. accumulate ----

@pytest.mark.parametrize("name,hash_", HASHES, ids=HASH_IDS)
def test_accumulate_basic(ctx, name, hash_):
    Rk, Sk = basic_case()
    rng = np.random.default_rng(3)
    vals = rng.integers(-2**63, 2**63 - 1, len(Sk))
    ctx.upload_columns(R_, Rk)
    with ctx.build_index(params_of(hash_), ordinals=True) as ix:
        check_acc(ctx, ix, Rk, Sk)                                   # counts only
        for stride in (1, 2):
            for vstride in (1, 2):
                check_acc(ctx, ix, Rk, Sk, values=vals, stride=stride, vstride=vstride)
        counts, sums, missing = ix.accumulate_host(Sk, vals)
        ec, es, em = expected_groups(Rk, Sk, vals)
        assert np.array_equal(counts, ec) and np.array_equal(sums.view(np.uint64), es) and missing == em
        counts, sums, missing = ix.accumulate_host(Sk)
        assert np.array_equal(counts, ec) and sums is None and missing == em


@pytest.mark.parametrize("name,hash_", HASHES, ids=HASH_IDS)
def test_accumulate_sums_wrap(ctx, name, hash_):
    Rk, Sk = basic_case()
    Sk = Sk[:30_000]
    vals = np.where(np.arange(len(Sk)) % 3 == 0, -2**62, 2**62).astype(np.int64)
    ctx.upload_columns(R_, Rk)
    with ctx.build_index(params_of(hash_), ordinals=True) as ix:
        assert (expected_groups(Rk, Sk)[0] > 4).any()               # 2^62 added more than four times wraps
        check_acc(ctx, ix, Rk, Sk, values=vals)


@pytest.mark.parametrize("name,hash_", HASHES, ids=HASH_IDS)
def test_accumulate_sizes_and_one_hot_key(ctx, name, hash_):
    Rk, Sk = basic_case()
    rng = np.random.default_rng(4)
    big = rng.integers(1, 2_300, 100_001)
    ctx.upload_columns(R_, Rk)
    with ctx.build_index(params_of(hash_), ordinals=True) as ix:
        for n in (1, 255, 1024, 1025, 100_001):
            check_acc(ctx, ix, Rk, big[:n], values=big[:n] * 1_000_003)
        hot = np.full(100_000, Rk[17], dtype=np.int64)
        check_acc(ctx, ix, Rk, hot, values=np.arange(100_000) - 50_000)
        check_acc(ctx, ix, Rk, np.full(100_000, 5_000_000), values=np.arange(100_000))   # and one absent key


@pytest.mark.parametrize("name,hash_", HASHES, ids=HASH_IDS)
def test_accumulate_cache_collisions(ctx, name, hash_):
    """Ordinals 5 and 5 + 2^k alternate: whatever power-of-two function of the
    ordinal picks the cache entry, some k sends both to one entry, so one of
    them owns it and the other adds with global atomics."""
    rng = np.random.default_rng(6)
    Rk = rng.permutation(20_000).astype(np.int64) * 3 + 7              # all distinct: ordinal == row
    ctx.upload_columns(R_, Rk)
    with ctx.build_index(params_of(hash_), ordinals=True) as ix:
        assert ix.info().distinct == 20_000
        for k in range(15):
            Sk = np.where(np.arange(20_000) % 2 == 0, Rk[5], Rk[5 + 2**k])
            vals = np.arange(20_000, dtype=np.int64) * 7 - 3
            d = 20_000
            acc = Acc("coll", d)
            acc.add(ix, "coll", Sk, vals)
            ctx.synchronize()
            counts, sums, missing = acc.results()
            ec, es, em = expected_groups(Rk, Sk, vals)
            assert ec[5] == ec[5 + 2**k] == 10_000 and em == 0
            assert np.array_equal(counts, ec) and np.array_equal(sums, es) and missing == 0, k


@functools.lru_cache(maxsize=None)
def zipf_case():
    R, S = O.generate_tables(30_000, 250_001, 1.05, 515)
    return np.ascontiguousarray(R[:, 0]), np.ascontiguousarray(S[:, 0]), np.ascontiguousarray(S[:, 1])


@pytest.mark.parametrize("name,hash_", HASHES, ids=HASH_IDS)
def test_accumulate_zipf_and_successive_batches(ctx, name, hash_):
    Rk, Sk, Sv = zipf_case()
    rng = np.random.default_rng(8)
    Rk = rng.permutation(Rk)                                            # ordinal != key order
    Sk = np.where(np.arange(len(Sk)) % 11 == 0, Sk + 10_000_000, Sk)    # some keys miss
    ctx.upload_columns(R_, Rk)
    with ctx.build_index(params_of(hash_), ordinals=True) as ix:
        assert np.bincount(expected_codes(Rk, Sk).clip(0)).max() > 5_000    # a hot group
        check_acc(ctx, ix, Rk, Sk, values=Sv, slot="zipf")
        # two batches in succession into the same accumulators
        acc = Acc("zipf2", len(Rk))
        acc.add(ix, "zipf2a", Sk[:100_000], Sv[:100_000])
        acc.add(ix, "zipf2b", Sk[100_000:], Sv[100_000:], stride=2, vstride=2)
        ctx.synchronize()
        counts, sums, missing = acc.results()
        ec, es, em = expected_groups(Rk, Sk, Sv)
        assert np.array_equal(counts, ec) and np.array_equal(sums, es) and missing == em
