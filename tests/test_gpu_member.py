"""phj_join_member on the GPU: which rows have a partner, as masks in input
order. The expectation is always numpy (np.isin), never the library. Every
mask is a preallocated device buffer filled with 0xFF between 0xA5 canaries."""
import ctypes as C
import functools

import numpy as np
import pytest

import partitionedhashjoin_amd as phj
from partitionedhashjoin_amd import _capi
from hashinv import preimage
from test_gpu_parity import edge_keys

pytestmark = pytest.mark.gpu
R_, S_ = phj.SIDE_BUILD, phj.SIDE_PROBE
GUARD = 64          # canary bytes on each side of a mask
BOTH = phj.MEMBER_PROBE | phj.MEMBER_BUILD
PARAMS = [("nopart-xxh3", phj.nopart_params()),
          ("nopart-murmur3", phj.nopart_params(hash=phj.HASH_MURMUR3)),
          ("radix88-murmur3", phj.radix_params((8, 8))),
          ("radix88-xxh3", phj.radix_params((8, 8), hash=phj.HASH_XXH3))]
PARAM_IDS = [a for a, _ in PARAMS]


class DevMask:
    """n mask bytes on the device at `offset` bytes past a 64-byte aligned
    address, 0xFF, with 0xA5 everywhere around them. The memory is the key
    column of a scratch context (the C ABI has no allocator)."""
    _donors = {}

    def __init__(self, slot, n, offset=0):
        self.n, self.lo = n, GUARD + offset
        total = self.lo + n + GUARD
        buf = np.full((total + 7) // 8 * 8, 0xA5, dtype=np.uint8)
        buf[self.lo:self.lo + n] = 0xFF
        self.before = buf
        d = DevMask._donors.get(slot)
        if d is None:
            d = DevMask._donors[slot] = phj.Context(0)
        self.d = d
        d.upload_columns(S_, buf.view(np.int64))
        base = d.columns_ptr(S_)[0]
        assert base % 64 == 0
        self.ptr = base + self.lo

    def read(self):
        """The n mask bytes; asserts that nothing else changed."""
        got = np.ascontiguousarray(self.d.download(S_)[:, 0]).view(np.uint8)
        out = got[self.lo:self.lo + self.n].copy()
        got[self.lo:self.lo + self.n] = 0xFF
        assert np.array_equal(got, self.before), "a byte outside [0, n) was written"
        return out


def member(ctx, params, sides=BOTH, po=0, bo=0):
    """(JoinResult, MemberCounts, probe mask bytes or None, build mask bytes or None) over the bound relations."""
    nS, nR = ctx.relation_ptr(S_)[1], ctx.relation_ptr(R_)[1]
    pm = DevMask("probe", nS, po) if sides & phj.MEMBER_PROBE else None
    bm = DevMask("build", nR, bo) if sides & phj.MEMBER_BUILD else None
    r, n, a, b = ctx.join_member(params, probe=pm is not None, build=bm is not None,
                                 probe_mask_ptr=pm.ptr if pm else None, build_mask_ptr=bm.ptr if bm else None)
    assert a is None and b is None
    return r, n, pm.read() if pm else None, bm.read() if bm else None


def check(ctx, params, Rk, Sk, sides=BOTH, po=0, bo=0):
    """The masks of the bound relations (keys Rk, Sk) equal np.isin both ways."""
    Rk, Sk = np.asarray(Rk, dtype=np.int64), np.asarray(Sk, dtype=np.int64)
    exp_s, exp_r = np.isin(Sk, Rk), np.isin(Rk, Sk)
    r, n, pm, bm = member(ctx, params, sides, po, bo)
    assert r.matches == n.probe_matched == int(exp_s.sum())
    if pm is not None:
        assert set(np.unique(pm)) <= {0, 1}
        assert np.array_equal(pm.astype(bool), exp_s)
    if bm is not None:
        assert set(np.unique(bm)) <= {0, 1}
        assert np.array_equal(bm.astype(bool), exp_r)
        assert n.build_matched == int(exp_r.sum())
    else:
        assert n.build_matched == 0
    return r, n


def tuples(keys, pay=0):
    keys = np.asarray(keys, dtype=np.int64)
    return np.stack([keys, np.full(len(keys), pay, dtype=np.int64) + np.arange(len(keys))], axis=1)


def bind(ctx, Rk, Sk):
    ctx.upload(R_, tuples(Rk, 1000))
    ctx.upload(S_, tuples(Sk, 5000))


@functools.lru_cache(maxsize=None)
def basic_case():
    rng = np.random.default_rng(77)
    Rk = rng.integers(1, 2_000, 3_000)                     # repeated build keys
    Sk = rng.integers(1, 2_300, 50_000)                    # about a third of them miss
    Rk.setflags(write=False)
    Sk.setflags(write=False)
    return Rk, Sk


# ---- basic ----

@pytest.mark.parametrize("sides", [1, 2, 3])
@pytest.mark.parametrize("name,params", PARAMS, ids=PARAM_IDS)
def test_member_basic(ctx, name, params, sides):
    Rk, Sk = basic_case()
    miss = 1 - np.isin(Sk, Rk).mean()
    assert 0.25 < miss < 0.45 and len(np.unique(Rk)) < len(Rk)
    bind(ctx, Rk, Sk)
    r, n = check(ctx, params, Rk, Sk, sides)
    assert n.probe_matched == ctx.join(phj.nopart_params(hash=params.hash)).matches
    names = [t[0] for t in r.timers()]
    assert "member.probe" in names and ("member.build" in names) == bool(sides & 2)
    assert "np.build" in names and "R.p1.hist" in names and r.algorithmic_bytes > 0


def test_member_allocating_form(ctx):
    Rk, Sk = basic_case()
    bind(ctx, Rk, Sk)
    r, n, pm, bm = ctx.join_member(phj.nopart_params(), probe=True, build=True)
    assert pm.dtype == bool and bm.dtype == bool
    assert np.array_equal(pm, np.isin(Sk, Rk)) and np.array_equal(bm, np.isin(Rk, Sk))
    r, n, pm, bm = ctx.join_member(phj.nopart_params(), probe=True, build=False)
    assert bm is None and np.array_equal(pm, np.isin(Sk, Rk)) and n.build_matched == 0


# ---- bindings ----

TRAP = 7   # a payload value that is also a key of both relations


@pytest.mark.parametrize("binding", ["tuples", "columns", "keys"])
@pytest.mark.parametrize("name,params", PARAMS[:2], ids=PARAM_IDS[:2])
def test_member_bindings(ctx, name, params, binding):
    Rk, Sk = basic_case()
    assert TRAP in Rk and TRAP in Sk
    donors = []
    try:
        if binding == "tuples":
            ctx.upload(R_, np.stack([Rk, np.full(len(Rk), TRAP)], axis=1))
            ctx.upload(S_, np.stack([Sk, np.full(len(Sk), TRAP)], axis=1))
        elif binding == "columns":
            ctx.upload_columns(R_, Rk, np.full(len(Rk), TRAP, dtype=np.int64))
            ctx.upload_columns(S_, Sk, np.full(len(Sk), TRAP, dtype=np.int64))
        else:
            # a key column alone inside a larger guarded buffer, 8-byte but not
            # 16-byte aligned; the guards hold a key of both sides, so an
            # over-read changes the answer
            guard = np.full(3, TRAP, dtype=np.int64)
            for side, k in ((R_, Rk), (S_, Sk)):
                d = phj.Context(0)
                donors.append(d)
                d.upload_columns(S_, np.concatenate([guard, k, guard]))
                base = d.columns_ptr(S_)[0]
                assert base % 16 == 0 and (base + 8 * len(guard)) % 16 == 8
                ctx.bind_columns(side, base + 8 * len(guard), None, len(k), keepalive=d)
        before = [ctx.relation_info(s).as_dict() for s in (R_, S_)]
        r, n = check(ctx, params, Rk, Sk)
        assert [ctx.relation_info(s).as_dict() for s in (R_, S_)] == before
        assert all(i["packed"] == 0 for i in before)
        assert not [t for t in r.timers() if t[0].endswith(".pack")]
        per = {t[0]: t[2] for t in r.timers()}
        assert per["R.p1.hist"] == len(Rk) * (16 if binding == "tuples" else 8)
    finally:
        bind(ctx, [1], [1])   # (rebinding releases the donors)
        for d in donors:
            d.close()


def test_member_payload_trap_is_not_read(ctx):
    # keys that nobody shares, payloads that everybody shares: all 0 both ways
    Rk, Sk = np.arange(1, 2_001, dtype=np.int64), np.arange(10_001, 15_001, dtype=np.int64)
    ctx.upload_columns(R_, Rk, Sk[:2_000].copy())
    ctx.upload_columns(S_, Sk, np.resize(Rk, 5_000))
    check(ctx, phj.nopart_params(), Rk, Sk)
    ctx.upload(R_, np.stack([Rk, Sk[:2_000]], axis=1))
    ctx.upload(S_, np.stack([Sk, np.resize(Rk, 5_000)], axis=1))
    check(ctx, phj.nopart_params(), Rk, Sk)


# ---- edges of the write ----

@pytest.mark.parametrize("nR", [1, 2, 300, 301, 1201])
def test_member_write_edges(ctx, nR):
    rng = np.random.default_rng(nR)
    Rk = rng.integers(1, max(2, nR), nR)
    p = phj.nopart_params()
    ctx.upload_columns(R_, Rk)
    for nS in (1, 63, 64, 65, 1023, 1024, 1025, 4097):
        Sk = rng.integers(1, 2 * max(2, nR), nS)
        ctx.upload_columns(S_, Sk)
        for off in (0, 3):
            check(ctx, p, Rk, Sk, BOTH, po=off, bo=off)


# ---- walks and the wrap ----

@pytest.mark.parametrize("name,params", PARAMS[:2], ids=PARAM_IDS[:2])
def test_member_walks_and_wrap(ctx, name, params):
    low = 0x2ABCD5                                     # 22 bits: the region, whatever the region count
    codes = [low | (0x1FFFF << 24) | (t << 41) for t in range(1, 9)]
    assert len(set(codes)) == 8 >= 6
    assert len({c & ((1 << 22) - 1) for c in codes}) == 1
    assert all((c >> 24) & 0x1FFFF == 0x1FFFF for c in codes)   # the last home bucket for any cap up to 2^18 slots
    mur = params.hash == phj.HASH_MURMUR3
    keys = np.array([preimage(mur, c, params.hash_seed) for c in codes], dtype=np.int64)
    assert len(np.unique(keys)) == 8
    got = phj.Context.hash_keys(ctx, params.hash, params.hash_seed, keys)
    assert [int(x) for x in got] == codes
    filler = np.arange(1, 601, dtype=np.int64)
    filler = filler[~np.isin(filler, keys)]
    Rk = np.concatenate([filler[:300], keys[::2], filler[300:]])      # half of the keys: two fill the bucket, two wrap
    Sk = np.concatenate([keys, filler[::2], keys[::-1], -filler[:50]])
    ctx.upload_columns(R_, Rk)
    ctx.upload_columns(S_, Sk)
    check(ctx, params, Rk, Sk)


# ---- empty-value preimages ----

@pytest.mark.parametrize("name,params", PARAMS, ids=PARAM_IDS)
def test_member_empty_value_preimages(ctx, name, params):
    pre = edge_keys(params)
    base = np.arange(1, 20_001, dtype=np.int64)
    base = base[~np.isin(base, pre)]
    Sk = np.concatenate([pre, base[::3], pre[::-1], -base[:500]])
    ctx.upload_columns(S_, Sk)
    ctx.upload_columns(R_, base)
    r, n, pm, bm = member(ctx, params)
    assert not pm[:len(pre)].any() and not pm[len(pre) + len(base[::3]):].any()   # in S only: all 0
    without = pm.copy()
    assert np.array_equal(pm.astype(bool), np.isin(Sk, base)) and np.array_equal(bm.astype(bool), np.isin(base, Sk))
    Rk = np.concatenate([base, pre, pre[:5]])
    ctx.upload_columns(R_, Rk)
    r, n, pm, bm = member(ctx, params)
    planted = np.isin(Sk, pre)
    assert pm[planted].all() and bm[len(base):].all()                             # in R too: all 1
    assert np.array_equal(pm[~planted], without[~planted])                        # nobody else's answer changes
    assert np.array_equal(pm.astype(bool), np.isin(Sk, Rk)) and np.array_equal(bm.astype(bool), np.isin(Rk, Sk))


# ---- non-uniform layout, repeated build keys, a hot probe key ----

@pytest.mark.parametrize("name,params", PARAMS[:2], ids=PARAM_IDS[:2])
def test_member_repeated_build_key(ctx, name, params):
    # one key 3000 times among 2000 others: its region is far above the
    # others', so the plan declines the uniform layout and desc[] is read
    others = np.arange(1, 2_001, dtype=np.int64)
    Rk = np.concatenate([others[:1000], np.full(3_000, 424_242, dtype=np.int64), others[1000:]])
    Sk = np.concatenate([others[::2], [424_242], -others[:300]])
    ctx.upload_columns(R_, Rk)
    ctx.upload_columns(S_, Sk)
    r, n, pm, bm = member(ctx, params)
    assert bm[1000:4000].all()
    assert np.array_equal(bm.astype(bool), np.isin(Rk, Sk)) and np.array_equal(pm.astype(bool), np.isin(Sk, Rk))
    assert n.build_matched == 3_000 + 1_000 and n.probe_matched == 1_001
    # and when nobody asks for the repeated key, none of its rows reads 1
    ctx.upload_columns(S_, Sk[Sk != 424_242])
    check(ctx, params, Rk, Sk[Sk != 424_242])


@pytest.mark.parametrize("name,params", PARAMS[:2], ids=PARAM_IDS[:2])
def test_member_hot_probe_key(ctx, name, params):
    Rk = np.arange(1, 3_001, dtype=np.int64)
    Sk = np.full(50_000, 1234, dtype=np.int64)
    ctx.upload_columns(R_, Rk)
    ctx.upload_columns(S_, Sk)
    r, n = check(ctx, params, Rk, Sk)
    assert (n.probe_matched, n.build_matched) == (50_000, 1)


# ---- marks do not leak ----

def _two_calls(c):
    Rk = np.arange(1, 5_001, dtype=np.int64)
    c.upload_columns(R_, Rk)
    for Sk in (np.arange(1, 2_001, dtype=np.int64), np.arange(3_001, 4_001, dtype=np.int64)):   # disjoint
        c.upload_columns(S_, Sk)
        r, n = check(c, phj.nopart_params(), Rk, Sk)
        assert n.build_matched == len(Sk)


def test_member_marks_do_not_leak(ctx):
    _two_calls(ctx)


def test_member_marks_under_poisoned_workspace():
    with phj.Context(0) as c:
        c.debug_poison_alloc(0xFF)
        _two_calls(c)


# ---- empty sides ----

def test_member_empty_sides(ctx):
    p = phj.nopart_params()
    k = np.arange(1, 1_001, dtype=np.int64)
    none = np.zeros(0, dtype=np.int64)
    for Rk, Sk in ((none, k), (k, none), (none, none)):
        ctx.upload_columns(R_, Rk)
        ctx.upload_columns(S_, Sk)
        r, n, pm, bm = member(ctx, p, BOTH, po=3, bo=3)
        assert (r.matches, n.probe_matched, n.build_matched) == (0, 0, 0)
        assert len(pm) == len(Sk) and not pm.any() and len(bm) == len(Rk) and not bm.any()
        # an empty relation's mask may be NULL
        pm, bm = DevMask("probe", len(Sk)), DevMask("build", len(Rk))
        rc, _ = raw(ctx, p, BOTH, pm.ptr if len(Sk) else 0, bm.ptr if len(Rk) else 0)
        assert rc == _capi.PHJ_OK
        assert not pm.read().any() and not bm.read().any()


# ---- bad arguments ----

def raw(c, params, sides, pptr, bptr):
    r, n = phj.JoinResult(), phj.MemberCounts()
    rc = c._L.phj_join_member(c._h, C.byref(params), sides, C.c_void_p(pptr), C.c_void_p(bptr), C.byref(r), C.byref(n))
    return rc, c._L.phj_last_error(c._h).decode()


def test_member_bad_arguments(ctx):
    Rk, Sk = basic_case()
    bind(ctx, Rk, Sk)
    p = phj.nopart_params()
    pm, bm = DevMask("probe", len(Sk)), DevMask("build", len(Rk))
    for sides in (0, 4, 1 << 31):
        assert raw(ctx, p, sides, pm.ptr, bm.ptr)[0] == _capi.PHJ_ERR_INVALID
    assert raw(ctx, p, phj.MEMBER_PROBE, 0, bm.ptr)[0] == _capi.PHJ_ERR_INVALID
    assert raw(ctx, p, phj.MEMBER_BUILD, pm.ptr, 0)[0] == _capi.PHJ_ERR_INVALID
    assert raw(ctx, p, BOTH, pm.ptr, 0)[0] == _capi.PHJ_ERR_INVALID
    assert raw(ctx, p, phj.MEMBER_PROBE, pm.ptr, 0)[0] == _capi.PHJ_OK      # a side that is not asked may be NULL
    bad = phj.nopart_params()
    bad.hash = 9
    assert raw(ctx, bad, BOTH, pm.ptr, bm.ptr)[0] == _capi.PHJ_ERR_INVALID
    assert raw(ctx, phj.radix_params((0, 0)), BOTH, pm.ptr, bm.ptr)[0] == _capi.PHJ_ERR_INVALID
    with phj.Context(devices=[0, 0], flags=phj.CTX_LOCAL) as g:
        rc, msg = raw(g, p, BOTH, pm.ptr, bm.ptr)
        assert rc == _capi.PHJ_ERR_STATE and "single-device" in msg


# ---- leaves others alone ----

def test_member_leaves_other_results_alone(ctx):
    rng = np.random.default_rng(5)
    Rk, Sk = rng.integers(1, 1_500, 2_000), rng.integers(1, 2_500, 20_000)
    bind(ctx, Rk, Sk)
    np_p, rx_p = phj.nopart_params(), phj.radix_params((8, 8))
    ctx.join_rows(np_p, phj.FULL_OUTER)
    rows = ctx.joined()
    check(ctx, np_p, Rk, Sk)
    assert np.array_equal(ctx.joined(), rows) and len(rows) > 0
    ctx.join_indices(np_p, phj.FULL_OUTER)
    b, q = ctx.joined_indices()
    check(ctx, rx_p, Rk, Sk)
    b2, q2 = ctx.joined_indices()
    assert np.array_equal(b, b2) and np.array_equal(q, q2) and len(b) > 0
    ctx.join_aggregate(np_p, groups=True)
    groups = ctx.groups()
    check(ctx, np_p, Rk, Sk)
    assert np.array_equal(ctx.groups(), groups) and len(groups) == len(Rk)
    exact = int(np.isin(Sk, Rk).sum())
    assert ctx.join(np_p).matches == exact and ctx.join(rx_p).matches == exact
