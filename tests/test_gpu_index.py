"""The retained key index on the GPU (phj_index_build / phj_index_lookup): key
-> lowest build row, built once, looked up per batch. The expectation is always
numpy (np.unique + np.searchsorted), never the library. Every output is a
preallocated device buffer filled with 0xEE between 0xA5 canaries."""
import ctypes as C
import functools

import numpy as np
import pytest

import hashinv
import partitionedhashjoin_amd as phj
from partitionedhashjoin_amd import _capi
from hashinv import NP_EDGES, _keys_of, np_edge_keys, np_home
from test_gpu_parity import edge_keys

pytestmark = pytest.mark.gpu
R_, S_ = phj.SIDE_BUILD, phj.SIDE_PROBE
GUARD = 64          # canary bytes on each side of an output
HASHES = [("xxh3", phj.HASH_XXH3), ("murmur3", phj.HASH_MURMUR3)]
HASH_IDS = [a for a, _ in HASHES]
SPECIAL = [0, -1, -2**63, 2**63 - 1]
M64 = (1 << 64) - 1


def expected(Rk, Sk):
    """numpy's answer: the lowest row of R holding each key of S, or -1."""
    Rk, Sk = np.asarray(Rk, dtype=np.int64), np.asarray(Sk, dtype=np.int64)
    if len(Rk) == 0:
        return np.full(len(Sk), -1, dtype=np.int64)
    u, first = np.unique(Rk, return_index=True)
    pos = np.searchsorted(u, Sk)
    pos = np.minimum(pos, len(u) - 1)
    hit = u[pos] == Sk
    return np.where(hit, first[pos], -1).astype(np.int64)


_donors = {}


def donor(slot):
    d = _donors.get(slot)
    if d is None:
        d = _donors[slot] = phj.Context(0)
    return d


class DevOut:
    """nbytes output bytes on the device at `offset` bytes past a 64-byte
    aligned address, filled with `fill`, with 0xA5 everywhere around them (the
    DevMask idea of test_gpu_member.py for int64 rows, bytes and a counter).
    The memory is the key column of a scratch context (the C ABI has no
    allocator)."""

    def __init__(self, slot, nbytes, offset=0, fill=0xEE):
        self.n, self.lo, self.fill = nbytes, GUARD + offset, fill
        total = self.lo + nbytes + GUARD
        buf = np.full((total + 7) // 8 * 8, 0xA5, dtype=np.uint8)
        buf[self.lo:self.lo + nbytes] = fill
        self.before = buf
        self.d = donor(slot)
        self.d.upload_columns(S_, buf.view(np.int64))
        base = self.d.columns_ptr(S_)[0]
        assert base % 64 == 0
        self.ptr = base + self.lo

    def read(self):
        """The output bytes; asserts that nothing around them changed."""
        got = np.ascontiguousarray(self.d.download(S_)[:, 0]).view(np.uint8)
        out = got[self.lo:self.lo + self.n].copy()
        got[self.lo:self.lo + self.n] = self.fill
        assert np.array_equal(got, self.before), "a byte outside [0, n) was written"
        return out


def dev_keys(slot, keys):
    """Device address of a copy of the int64 array `keys` (0 when empty)."""
    d = donor(slot)
    d.upload_columns(R_, np.ascontiguousarray(keys, dtype=np.int64))
    return d.columns_ptr(R_)[0] or 0


class Job:
    """One lookup's inputs and guarded outputs, made before anything is enqueued."""

    def __init__(self, slot, Sk, stride=1, found_off=0, count=None):
        Sk = np.asarray(Sk, dtype=np.int64)
        self.n, self.stride = len(Sk), stride
        src = Sk if stride == 1 else np.stack([Sk, np.roll(Sk, 1)], axis=1).reshape(-1)   # payloads are keys too
        self.keys = dev_keys(slot + ".k", src)
        self.rows = DevOut(slot + ".r", 8 * self.n)
        self.found = DevOut(slot + ".f", self.n, found_off)
        self.count = count if count is not None else DevOut(slot + ".c", 8, fill=0)

    def enqueue(self, ix):
        ix.lookup(self.keys, self.n, self.rows.ptr, self.found.ptr, self.count.ptr, key_stride=self.stride)

    def results(self):
        return self.rows.read().view(np.int64), self.found.read()


def lookup(ctx, ix, Sk, stride=1, found_off=0, slot="a"):
    """(rows, found bytes, device count) of one lookup, canaries checked."""
    j = Job(slot, Sk, stride, found_off)
    j.enqueue(ix)
    ctx.synchronize()
    rows, found = j.results()
    return rows, found, int(j.count.read().view(np.uint64)[0])


def check(ctx, ix, Rk, Sk, **kw):
    exp = expected(Rk, Sk)
    rows, found, cnt = lookup(ctx, ix, Sk, **kw)
    assert set(np.unique(found)) <= {0, 1}
    bad = np.flatnonzero(rows != exp)
    assert len(bad) == 0, (len(bad), bad[:5], rows[bad[:5]], exp[bad[:5]])
    assert np.array_equal(found.astype(bool), exp >= 0)
    assert cnt == int((exp >= 0).sum())
    return exp


def tuples(keys, pay=0):
    keys = np.asarray(keys, dtype=np.int64)
    return np.stack([keys, np.full(len(keys), pay, dtype=np.int64) + np.arange(len(keys))], axis=1)


def params_of(hash_, ratio=0.0):
    return phj.nopart_params(hash=hash_, table_ratio=ratio)


@functools.lru_cache(maxsize=None)
def basic_case():
    rng = np.random.default_rng(77)
    Rk = rng.integers(1, 2_000, 3_000)                     # repeated build keys
    Sk = rng.integers(1, 2_300, 50_000)                    # about a third of them miss
    Rk.setflags(write=False)
    Sk.setflags(write=False)
    return Rk, Sk


# ---- basic ----

@pytest.mark.parametrize("name,hash_", HASHES, ids=HASH_IDS)
def test_index_basic(ctx, name, hash_):
    Rk, Sk = basic_case()
    miss = 1 - np.isin(Sk, Rk).mean()
    assert 0.25 < miss < 0.45 and len(np.unique(Rk)) < len(Rk)
    ctx.upload(R_, tuples(Rk, 1000))
    ctx.upload(S_, tuples(Sk, 5000))
    p = params_of(hash_)
    with ctx.build_index(p) as ix:
        info = ix.info()
        assert info.rows == len(Rk) and info.distinct == len(np.unique(Rk)) == ix.result.matches
        assert info.slots == 5 and 1 <= info.rbits <= 22 and info.nb == info.nbr << info.rbits
        assert info.table_bytes == info.nb * 64 and info.nb * info.slots >= 2 * len(Rk)
        names = [t[0] for t in ix.result.timers()]
        assert "index.build" in names and "R.p1.hist" in names and ix.result.algorithmic_bytes > 0
        assert not any(n.endswith(".pack") for n in names)
        exp = check(ctx, ix, Rk, Sk)
        assert int((exp >= 0).sum()) == ctx.join(phj.nopart_params(hash=hash_)).matches
        rows, found = ix.lookup_host(Sk[:1000])
        assert found.dtype == bool and np.array_equal(rows, exp[:1000]) and np.array_equal(found, exp[:1000] >= 0)


# ---- batch edges ----

@pytest.mark.parametrize("found_off", [0, 1, 3])
def test_index_batch_edges(ctx, found_off):
    Rk, Sk = basic_case()
    ctx.upload(R_, tuples(Rk))
    with ctx.build_index(params_of(phj.HASH_XXH3)) as ix:
        for n in (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4097):
            check(ctx, ix, Rk, Sk[1000:1000 + n], found_off=found_off)


# ---- stride 2 ----

@pytest.mark.parametrize("name,hash_", HASHES, ids=HASH_IDS)
def test_index_stride2_reads_ids_only(ctx, name, hash_):
    Rk, Sk = basic_case()
    Sk = Sk[:20_001]
    # Job's tuple array pairs each id with its neighbour's id: were a payload looked up, it would hit
    assert (expected(Rk, np.roll(Sk, 1)) != expected(Rk, Sk)).any()
    ctx.upload(R_, tuples(Rk))
    with ctx.build_index(params_of(hash_)) as ix:
        check(ctx, ix, Rk, Sk, stride=2)


# ---- binding at build ----

@pytest.mark.parametrize("name,hash_", HASHES, ids=HASH_IDS)
def test_index_bindings_at_build(ctx, name, hash_):
    Rk, Sk = basic_case()
    TRAP = 2_250   # a payload value that S looks up and R's keys lack
    assert TRAP not in Rk and TRAP in Sk
    p = params_of(hash_)
    answers = []
    for binding in ("tuples", "columns", "keys"):
        if binding == "tuples":
            ctx.upload(R_, np.stack([Rk, np.full(len(Rk), TRAP)], axis=1))
        elif binding == "columns":
            ctx.upload_columns(R_, Rk, np.full(len(Rk), TRAP, dtype=np.int64))
        else:
            ctx.upload_columns(R_, Rk)
        packed = ctx.relation_info(R_).packed
        with ctx.build_index(p) as ix:
            assert ctx.relation_info(R_).packed == packed == 0
            assert not any(t[0].endswith(".pack") for t in ix.result.timers())
            check(ctx, ix, Rk, Sk)
            answers.append(lookup(ctx, ix, Sk)[0])
    assert np.array_equal(answers[0], answers[1]) and np.array_equal(answers[0], answers[2])


# ---- edge keys ----

@pytest.mark.parametrize("name,hash_", HASHES, ids=HASH_IDS)
def test_index_edge_keys_present_and_absent(ctx, name, hash_):
    p = params_of(hash_)
    special = np.unique(np.concatenate([np.array(SPECIAL, dtype=np.int64), edge_keys(p)]))
    rng = np.random.default_rng(9)
    filler = np.setdiff1d(rng.integers(-2**62, 2**62, 700), special)[:600]
    # present: each special key at a known non-zero row among the fillers
    Rk = np.concatenate([filler[:100], special, filler[100:]])
    ctx.upload(R_, tuples(Rk))
    with ctx.build_index(p) as ix:
        exp = check(ctx, ix, Rk, np.concatenate([special, filler[:50]]))
        assert np.array_equal(exp[:len(special)], 100 + np.arange(len(special)))
        for k in SPECIAL:   # and one at a time
            check(ctx, ix, Rk, [k])
    # absent: the same lookups against the fillers alone must all miss
    ctx.upload(R_, tuples(filler))
    with ctx.build_index(p) as ix:
        exp = check(ctx, ix, filler, np.concatenate([special, filler[:50]]))
        assert (exp[:len(special)] == -1).all() and (exp[len(special):] >= 0).all()
        for k in SPECIAL:
            rows, found, cnt = lookup(ctx, ix, [k])
            assert rows[0] == -1 and found[0] == 0 and cnt == 0


# ---- hot build key ----

def test_index_hot_build_key(ctx):
    rng = np.random.default_rng(31)
    HOT = 777_777_777
    others = rng.permutation(np.arange(50_000, dtype=np.int64) * 13 + 1_000_000_000)
    Rk = np.empty(200_000, dtype=np.int64)
    pos = rng.permutation(np.arange(18, 200_000))     # row 17 is the hot key's first occurrence
    Rk[:17] = others[:17]
    Rk[17] = HOT
    Rk[pos[:149_999]] = HOT
    Rk[pos[149_999:]] = others[17:]
    assert (Rk == HOT).sum() == 150_000 and np.flatnonzero(Rk == HOT)[0] == 17
    Sk = np.concatenate([np.full(10_000, HOT), rng.choice(others, 10_000), rng.integers(1, 1_000_000, 10_000)])
    rng.shuffle(Sk)
    p = params_of(phj.HASH_XXH3)
    ctx.upload_columns(R_, Rk)
    with ctx.build_index(p) as ix:
        info = ix.info()
        assert info.distinct == 50_001
        exp = check(ctx, ix, Rk, Sk)
        assert (exp[Sk == HOT] == 17).all()
        hot_bytes = info.table_bytes
    ctx.upload_columns(R_, np.arange(200_000, dtype=np.int64))
    with ctx.build_index(p) as ix:
        assert hot_bytes <= ix.info().table_bytes


# ---- crafted collisions ----

@functools.lru_cache(maxsize=None)
def _inv_lin_columns():
    return np.array([hashinv._inv_lin(1 << i) for i in range(64)], dtype=np.uint64)


def keys_of_fast(ctx, params, codes):
    """hashinv._keys_of over many codes: the same inverses, vectorised (the
    per-key Gaussian elimination of xxh3_inverse takes milliseconds a key).
    Checked two ways: equal to _keys_of on a sample, and the device's own hash
    of every key is its code."""
    codes = np.asarray([c & M64 for c in codes], dtype=np.uint64)
    seed = params.hash_seed & M64
    u = np.uint64

    def inv_xs(y, s):
        x = y.copy()
        for _ in range(64 // s + 1):
            x = y ^ (x >> u(s))
        return x

    with np.errstate(over="ignore"):
        if params.hash == phj.HASH_MURMUR3:
            x = inv_xs(codes, 33)
            x = x * u(hashinv._inv_mul(0xC4CEB9FE1A85EC53))
            x = inv_xs(x, 33)
            x = x * u(hashinv._inv_mul(0xFF51AFD7ED558CCD))
            x = inv_xs(x, 33) ^ u(seed)
        else:
            Ci = u(hashinv._inv_mul(0x9FB21C651E98DF25))
            x = inv_xs(codes, 28) * Ci
            x = x ^ ((x >> u(35)) + u(8))
            x = x * Ci
            cols, y = _inv_lin_columns(), np.zeros_like(x)
            for i in range(64):   # the inverse of a linear map, column by column
                y ^= np.where((x >> u(i)) & u(1), cols[i], u(0))
            x = y ^ u(hashinv._xxh3_bitflip(seed))
            x = (x >> u(32)) | (x << u(32))
    keys = x.view(np.int64)
    assert np.array_equal(keys[:8], _keys_of(params, [int(c) for c in codes[:8]]))
    assert np.array_equal(ctx.hash_keys(params.hash, params.hash_seed, keys), codes)
    assert len(np.unique(keys)) == len(keys)
    return keys


@pytest.mark.parametrize("where", list(NP_EDGES))
@pytest.mark.parametrize("name,hash_", HASHES, ids=HASH_IDS)
def test_index_crafted_edge_buckets(ctx, name, hash_, where):
    """1024 keys homed at one bucket at a region's or the table's edge (the
    walk leaves the region; at the table's end it wraps), and 1024 absent keys
    with the same home. Bits 22..31 of a code count only to 1023, so the absent
    keys take a second high-word pattern, hi ^ 1: (hi' * nbr) >> 32 is the same
    bucket for every nbr <= 2^22, which np_home confirms below."""
    p = params_of(hash_)
    rng = np.random.default_rng(12)
    mates = np_edge_keys(p, where, 1024)
    hi, low = NP_EDGES[where]
    absent_codes = [((hi ^ 1) << 32) | (t << 22) | low for t in range(1024)]
    absent = _keys_of(p, absent_codes[:4])
    absent = np.concatenate([absent, keys_of_fast(ctx, p, absent_codes[4:])])
    rnd = np.setdiff1d(rng.integers(1, 2**40, 5_200), np.concatenate([mates, absent]))[:5_000]
    Rk = np.concatenate([rnd[:2_500], mates, rnd[2_500:]])
    rng.shuffle(Rk)
    ctx.upload_columns(R_, Rk)
    with ctx.build_index(p) as ix:
        info = ix.info()
        g = (info.nb, info.nbr, info.rbits)
        homes = np_home(ctx.hash_keys(p.hash, p.hash_seed, np.concatenate([mates, absent])), g)
        assert len(np.unique(homes)) == 1
        assert info.distinct == len(Rk)
        Sk = np.concatenate([Rk, absent])
        rng.shuffle(Sk)
        exp = check(ctx, ix, Rk, Sk)
        assert (exp >= 0).sum() == len(Rk)


@pytest.mark.parametrize("name,hash_", HASHES, ids=HASH_IDS)
def test_index_one_region_far_beyond_its_share(ctx, name, hash_):
    """20,000 distinct keys whose codes end in 22 zero bits: all of region 0,
    many times what its LDS table holds; the rest go through the overflow pass
    into the following regions."""
    p = params_of(hash_)
    rng = np.random.default_rng(13)
    crowd = keys_of_fast(ctx, p, [(((t * 0x9E3779B1) & 0xFFFFFFFF) << 32) for t in range(20_000)])
    rnd = np.setdiff1d(rng.integers(1, 2**40, 2_100), crowd)[:2_000]
    Rk = np.concatenate([crowd, rnd])
    rng.shuffle(Rk)
    ctx.upload_columns(R_, Rk)
    with ctx.build_index(p) as ix:
        info = ix.info()
        assert info.distinct == len(Rk) and info.nbr * info.slots < 20_000
        Sk = np.concatenate([Rk, rng.integers(2**41, 2**42, 5_000)])
        rng.shuffle(Sk)
        check(ctx, ix, Rk, Sk)


# ---- retention ----

def test_index_is_retained(ctx):
    rng = np.random.default_rng(21)
    R1 = rng.integers(1, 30_000, 20_000)
    R2 = rng.integers(20_000, 60_000, 25_000)
    Sk = rng.integers(1, 70_000, 100_000)
    p = params_of(phj.HASH_XXH3)
    ctx.upload(R_, tuples(R1))
    ctx.upload(S_, tuples(Sk))
    ix1 = ctx.build_index(p)
    try:
        check(ctx, ix1, R1, Sk)
        ctx.upload(R_, tuples(R2))                      # rebind the build side
        assert ctx.join(p).matches == int(np.isin(Sk, R2).sum())
        r, n, pm, bm = ctx.join_member(p, probe=True, build=True)
        assert np.array_equal(pm, np.isin(Sk, R2)) and np.array_equal(bm, np.isin(R2, Sk))
        r, n = ctx.join_indices(p, phj.PROBE_OUTER)
        b, s = ctx.joined_indices()
        u, cnt = np.unique(R2, return_counts=True)
        per = np.where(np.isin(Sk, u), cnt[np.minimum(np.searchsorted(u, Sk), len(u) - 1)], 0)
        assert n.pairs == int(per.sum()) and n.probe_only == int((per == 0).sum())
        assert np.array_equal(s, np.repeat(np.arange(len(Sk)), np.maximum(per, 1)))
        hit = b >= 0
        assert np.array_equal(R2[b[hit]], Sk[s[hit]]) and np.array_equal(hit, np.repeat(per > 0, np.maximum(per, 1)))
        check(ctx, ix1, R1, Sk)                         # still R1's answers
        ix2 = ctx.build_index(params_of(phj.HASH_MURMUR3))
        try:
            check(ctx, ix2, R2, Sk)
            check(ctx, ix1, R1, Sk)
        finally:
            ix1.close()                                 # the older one first ...
            check(ctx, ix2, R2, Sk)
            ix2.close()
        with pytest.raises(phj.PhjError):
            ix1.info()
    finally:
        ix1.close()
    # ... and the newer one first; closing a context with an index open frees it
    with phj.Context(0) as c:
        c.upload_columns(R_, R1)
        a, b = c.build_index(p), c.build_index(p)
        b.close()
        check(c, a, R1, Sk[:5_000], slot="own")
        a.close()
        left = c.build_index(p)
    with pytest.raises(phj.PhjError):
        left.info()
    left.close()


# ---- poisoned workspace ----

@pytest.mark.parametrize("byte", [0xFF, 0x00])
def test_index_poisoned_workspace(byte):
    Rk, Sk = basic_case()
    with phj.Context(0) as c:
        c.debug_poison_alloc(byte)
        c.upload(R_, tuples(Rk))
        for hash_ in (phj.HASH_XXH3, phj.HASH_MURMUR3):
            with c.build_index(params_of(hash_)) as ix:
                assert ix.info().distinct == len(np.unique(Rk))
                check(c, ix, Rk, Sk, slot="poison")


# ---- enqueue only ----

def test_index_lookups_are_enqueued(ctx):
    Rk, Sk = basic_case()
    ctx.upload(R_, tuples(Rk))
    shared = DevOut("enq.count", 8, fill=0)
    cuts = [0, 700, 5_000, 5_001, 12_345, 20_000, 33_333, 41_000, 50_000]
    with ctx.build_index(params_of(phj.HASH_MURMUR3)) as ix:
        jobs = [Job(f"enq{i}", Sk[cuts[i]:cuts[i + 1]], found_off=i % 4, count=shared) for i in range(8)]
        for j in jobs:          # back to back, no call in between
            j.enqueue(ix)
        ctx.synchronize()
        total = 0
        for i, j in enumerate(jobs):
            exp = expected(Rk, Sk[cuts[i]:cuts[i + 1]])
            rows, found = j.results()
            assert np.array_equal(rows, exp) and np.array_equal(found.astype(bool), exp >= 0)
            total += int((exp >= 0).sum())
        assert int(shared.read().view(np.uint64)[0]) == total


# ---- errors ----

def test_index_errors(ctx):
    Rk, Sk = basic_case()
    ctx.upload(R_, tuples(Rk))
    keys = dev_keys("err.k", Sk[:100])
    rows = DevOut("err.r", 8 * 100)
    with ctx.build_index(params_of(phj.HASH_XXH3)) as ix:
        def code(*a, **kw):
            with pytest.raises(phj.PhjError) as e:
                ix.lookup(*a, **kw)
            return e.value.code
        for stride in (0, 3):
            assert code(keys, 100, rows.ptr, key_stride=stride) == _capi.PHJ_ERR_INVALID
        assert code(keys + 4, 50, rows.ptr) == _capi.PHJ_ERR_INVALID
        assert code(keys, 50, rows.ptr + 4) == _capi.PHJ_ERR_INVALID
        assert code(keys, 50, None) == _capi.PHJ_ERR_INVALID
        assert code(None, 50, rows.ptr) == _capi.PHJ_ERR_INVALID
        ix.lookup(keys, 0, rows.ptr)            # n == 0: nothing is launched or written
        ix.lookup(None, 0, None)
        ctx.synchronize()
        assert (rows.read() == 0xEE).all()
        with phj.Context(0) as other:           # an index belongs to its context
            with pytest.raises(phj.PhjError) as e:
                other._check(other._L.phj_index_lookup(other._h, ix._h, C.c_void_p(keys), 1, 10,
                                                       C.c_void_p(rows.ptr), None, None))
            assert e.value.code == _capi.PHJ_ERR_INVALID
        assert (rows.read() == 0xEE).all()
    bad_algo = params_of(phj.HASH_XXH3)
    bad_algo.algo = 9
    for bad in (bad_algo, params_of(7), params_of(phj.HASH_XXH3, 0.5), phj.radix_params((12, 12))):
        with pytest.raises(phj.PhjError) as e:
            ctx.build_index(bad)
        assert e.value.code == _capi.PHJ_ERR_INVALID
    with phj.Context(devices=[0, 0], flags=phj.CTX_LOCAL) as g:
        with pytest.raises(phj.PhjError, match="single-device") as e:
            g.build_index(params_of(phj.HASH_XXH3))
        assert e.value.code == _capi.PHJ_ERR_STATE


def test_index_over_an_empty_build_side(ctx):
    _, Sk = basic_case()
    ctx.upload_columns(R_, np.zeros(0, dtype=np.int64))
    with ctx.build_index(params_of(phj.HASH_XXH3)) as ix:
        info = ix.info()
        assert info.rows == 0 and info.distinct == 0 and ix.result.matches == 0
        exp = check(ctx, ix, [], np.concatenate([Sk[:3_000], np.array(SPECIAL, dtype=np.int64)]))
        assert (exp == -1).all()


# ---- mid size ----

@functools.lru_cache(maxsize=None)
def mid_case():
    rng = np.random.default_rng(5)
    Rk = rng.permutation(2_000_000)[:1_000_000].astype(np.int64) * 7 + 3      # shuffled, distinct
    Sk = np.where(rng.random(4_000_000) < 0.5, rng.choice(Rk, 4_000_000), rng.integers(0, 2**40, 4_000_000) * 7 + 4)
    return Rk, Sk, expected(Rk, Sk)


@pytest.mark.parametrize("ratio", [0.0, 1.0])
def test_index_mid_size(ctx, ratio):
    Rk, Sk, exp = mid_case()
    assert len(np.unique(Rk)) == len(Rk) and 0.45 < (exp < 0).mean() < 0.55
    ctx.upload_columns(R_, Rk)
    with ctx.build_index(params_of(phj.HASH_XXH3, ratio)) as ix:
        info = ix.info()
        assert info.distinct == len(Rk) and info.nb * info.slots >= len(Rk)
        rows, found, cnt = lookup(ctx, ix, Sk, slot="mid")
        assert np.array_equal(rows, exp) and np.array_equal(found.astype(bool), exp >= 0) and cnt == int((exp >= 0).sum())
