"""Relations bound as a key column and a payload column (phj_relation_*_columns).

The counting LDS join in its default schedule reads the key column itself
(k_chunk_codes_pipe COLS, k_hot_sample COLS): the count is the oracle's, no
tuple copy is made (relation_info.packed == 0, no `*.pack` timer) and pass 1
is accounted 8 B per tuple less than on tuples. Every other call packs the
side once and gives what the same data bound as tuples gives.
"""
import functools

import numpy as np
import pytest

import partitionedhashjoin_amd as phj
from partitionedhashjoin_amd import _capi
from oracle import oracle as O

pytestmark = pytest.mark.gpu

NR = 1_000_000
NS = 3_000_000
TAIL = 1237          # a partial last tile, and an odd column
MUR, XXH = phj.HASH_MURMUR3, phj.HASH_XXH3
R_, S_ = phj.SIDE_BUILD, phj.SIDE_PROBE


def params(hk=MUR, flags=0):
    p = phj.radix_params((8, 8), hash=hk)
    p.flags |= flags
    return p


@pytest.fixture(scope="module")
def cols(ctx):
    """A context of its own without the hot-key pre-aggregation."""
    c = phj.Context(0)
    c.debug_preagg(phj.PREAGG_OFF)
    yield c
    c.close()


@pytest.fixture(scope="module")
def hot(ctx):
    """A context of its own with the pre-aggregation forced (as tests/test_gpu_preagg.py)."""
    c = phj.Context(0)
    c.debug_preagg(phj.PREAGG_FORCED)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def zipf_s(alpha, seed=77):
    return O.fill_zipf(NS + TAIL, alpha, 1, NR, seed)


@functools.lru_cache(maxsize=None)
def seq_r(start, n=NR):
    return O.fill_sequential(n, start)


@functools.lru_cache(maxsize=None)
def expect_zipf(start, alpha, tail):
    return O.semijoin_count(seq_r(start), zipf_s(alpha)[:NS + tail])


@functools.lru_cache(maxsize=None)
def half_miss(n, hi=NR, seed=5):
    """n probe tuples with keys uniform over [1, 2 hi]: those above hi miss R = 1 .. hi."""
    rng = np.random.default_rng(seed + n)
    S = np.empty((n, 2), dtype=np.int64)
    S[:, 0] = rng.integers(1, 2 * hi + 1, size=n)
    S[:, 1] = np.arange(n) * 3 + 1
    return S


def up_cols(c, side, rel, payloads=True):
    c.upload_columns(side, rel[:, 0], rel[:, 1] if payloads else None)


def timer_names(r):
    return [t[0] for t in r.timers()]


def timer_bytes(r, name):
    return {t[0]: t[2] for t in r.timers()}[name]


def assert_native(c, r):
    assert c.relation_info(R_).packed == 0 and c.relation_info(S_).packed == 0
    assert not [n for n in timer_names(r) if n.endswith(".pack")], timer_names(r)


_tuple_bytes = {}


def tuple_scatter_bytes(ctx, nR, nS, hk):
    """(R.p1.scatter, S.p1.scatter) bytes of the same join bound as tuples (they depend on the sizes only)."""
    key = (nR, nS, hk)
    if key not in _tuple_bytes:
        ctx.upload(R_, seq_r(1)[:nR])
        ctx.upload(S_, zipf_s(1.05)[:nS])
        r = ctx.join(params(hk))
        _tuple_bytes[key] = (timer_bytes(r, "R.p1.scatter"), timer_bytes(r, "S.p1.scatter"))
    return _tuple_bytes[key]


# ---- count parity on the native path ----

@pytest.mark.parametrize("start", [1, 4], ids=["all-hit", "top3-miss"])
@pytest.mark.parametrize("hk", [MUR, XXH], ids=["murmur3", "xxh3"])
@pytest.mark.parametrize("alpha", [1.05, 1.25])
@pytest.mark.parametrize("tail", [0, TAIL])
@pytest.mark.parametrize("mode", ["off", "forced"])
def test_count_native(ctx, cols, hot, mode, tail, alpha, hk, start):
    c = cols if mode == "off" else hot
    R, S = seq_r(start), zipf_s(alpha)[:NS + tail]
    assert phj.join_path(params(hk), len(R), len(S)) == phj.PATH_LDS_JOIN
    up_cols(c, R_, R)
    up_cols(c, S_, S)
    expect = expect_zipf(start, alpha, tail)
    for _ in range(3):
        r = c.join(params(hk))
        assert r.matches == expect
        entries, agg = c.debug_preagg()
        if mode == "forced":
            assert entries > 0 and 0 < agg <= len(S), (entries, agg)
        else:
            assert (entries, agg) == (0, 0)
        assert_native(c, r)
    if mode == "off":
        rb, sb = tuple_scatter_bytes(ctx, len(R), len(S), hk)
        assert timer_bytes(r, "S.p1.scatter") == sb - 8 * len(S)
        assert timer_bytes(r, "R.p1.scatter") == rb - 8 * len(R)
    # as bench.py sets the flags: the timers stay in the context
    rd = c.join(params(hk, phj.DEFER_TIMERS | phj.LEAN_TIMERS))
    assert rd.matches == expect
    rep = c.timers_report()
    assert not [n for n in timer_names(rep) if n.endswith(".pack")]
    assert c.relation_info(S_).packed == 0 and c.relation_info(R_).packed == 0


# ---- tile edges ----

@pytest.mark.parametrize("mode", ["off", "forced"])
@pytest.mark.parametrize("ns", [1, 63, 64, 3000, 4095, 4096, 4097, 2 * 4096 + 1])
def test_probe_tile_edges(cols, hot, ns, mode):
    c = cols if mode == "off" else hot
    R, S = seq_r(1), half_miss(ns)
    assert phj.join_path(params(), len(R), ns) == phj.PATH_LDS_JOIN
    up_cols(c, R_, R)
    up_cols(c, S_, S, payloads=False)
    r = c.join(params())
    assert r.matches == O.semijoin_count(R, S)
    assert_native(c, r)


@pytest.mark.parametrize("mode", ["off", "forced"])
@pytest.mark.parametrize("nr", [1, 4097])
def test_build_tile_edges(cols, hot, nr, mode):
    c = cols if mode == "off" else hot
    R, S = seq_r(1, nr), half_miss(NS, hi=nr)
    assert phj.join_path(params(), nr, NS) == phj.PATH_LDS_JOIN
    up_cols(c, R_, R, payloads=False)
    up_cols(c, S_, S)
    r = c.join(params())
    assert r.matches == O.semijoin_count(R, S)
    assert_native(c, r)


# ---- a key column alone ----

def test_key_column_alone(ctx, cols):
    nR, nS = 100_000, 300_001
    R, S = seq_r(1, nR).copy(), half_miss(nS, hi=nR)
    R[5000:5003, 0] = 7     # duplicate build keys: pairs != matches
    ctx.upload(R_, R)
    ctx.upload(S_, S)
    p = params()
    want_pairs = ctx.join_inner_count(p).matches
    want_outer = ctx.join_rows_count(p, phj.FULL_OUTER)[1].as_dict()
    semi = O.semijoin_count(R, S)
    up_cols(cols, R_, R, payloads=False)
    up_cols(cols, S_, S, payloads=False)
    assert cols.relation_info(S_).has_payloads == 0
    assert cols.join(p).matches == semi
    assert cols.join_inner_count(p).matches == want_pairs
    assert cols.join_rows_count(p, phj.FULL_OUTER)[1].as_dict() == want_outer
    for call in (lambda: cols.join_inner(p), lambda: cols.join_rows(p, phj.FULL_OUTER),
                 lambda: cols.join_materialize(p), lambda: cols.join_aggregate(p)):
        with pytest.raises(phj.PhjError) as e:
            call()
        assert e.value.code == _capi.PHJ_ERR_STATE and "payload column" in str(e.value)
    assert cols.join(p).matches == semi
    assert cols.join(phj.nopart_params()).matches == semi


# ---- nothing outside the column is read; an 8-byte aligned base works ----

GUARD = 4099   # odd (the bound base is 8-B but not 16-B aligned) and more than a tile


@pytest.mark.parametrize("mode", ["off", "forced"])
@pytest.mark.parametrize("tail", [0, TAIL])
def test_guarded_column(cols, hot, tail, mode):
    c = cols if mode == "off" else hot
    R = seq_r(1)
    real = zipf_s(1.05)[:NS + tail, 0]
    guard = np.full(GUARD, 7, dtype=np.int64)      # a key R holds: an over-read raises the count
    donor = phj.Context(0)
    donor.upload_columns(S_, np.concatenate([guard, real, guard]))
    base = donor.columns_ptr(S_)[0]
    assert base % 16 == 0 and (base + 8 * GUARD) % 16 == 8
    up_cols(c, R_, R, payloads=False)
    c.bind_columns(S_, base + 8 * GUARD, None, len(real), keepalive=donor)
    info = c.relation_info(S_)
    assert (info.n, info.layout, info.has_payloads, info.owned) == (len(real), phj.LAYOUT_COLUMNS, 0, 0)
    for hk in (MUR, XXH):
        r = c.join(params(hk))
        assert r.matches == expect_zipf(1, 1.05, tail)
        assert_native(c, r)
    c.upload_columns(S_, real[:1])   # (rebinding releases the donor)
    donor.close()


@pytest.mark.parametrize("mode", ["off", "forced"])
def test_payload_stride_trap(cols, hot, mode):
    c = cols if mode == "off" else hot
    n = 300_001
    R, S = seq_r(1), half_miss(n)
    trap = np.full(n, 11, dtype=np.int64)          # what a 16-B stride would read from buf[n:2n]: all match
    donor = phj.Context(0)
    donor.upload_columns(S_, np.concatenate([S[:, 0], trap]))
    up_cols(c, R_, R, payloads=False)
    c.bind_columns(S_, donor.columns_ptr(S_)[0], None, n, keepalive=donor)
    r = c.join(params())
    assert r.matches == O.semijoin_count(R, S)
    assert_native(c, r)
    c.upload_columns(S_, S[:1, 0])
    donor.close()


# ---- phj_probe_pass1 on a columnar probe side ----

def by_digit(codes, b1):
    dig = np.repeat(np.arange(len(b1) - 1), np.diff(b1.astype(np.int64)))
    return codes[np.lexsort((codes, dig))]


@pytest.mark.parametrize("hk", [MUR, XXH], ids=["murmur3", "xxh3"])
def test_probe_pass1(ctx, cols, hk):
    R, S = seq_r(1), zipf_s(1.25)[:NS + TAIL]
    ctx.upload(R_, R)
    ctx.upload(S_, S)
    codes_t, b1_t, is_codes_t = ctx.probe_pass1(params(hk))
    up_cols(cols, R_, R)
    up_cols(cols, S_, S)
    codes_c, b1_c, is_codes_c = cols.probe_pass1(params(hk))
    assert is_codes_t and is_codes_c
    assert np.array_equal(b1_c, b1_t)
    assert np.array_equal(by_digit(codes_c, b1_c), by_digit(codes_t, b1_t))
    assert cols.relation_info(S_).packed == 0


# ---- fallback: one packed copy ----

def sorted_rows(a):
    return a[np.lexsort(a.T[::-1])]


def test_fallback_packs_once(ctx, cols):
    nR, nS = 100_000, 300_001
    R, S = seq_r(1, nR), half_miss(nS, hi=nR)
    ctx.upload(R_, R)
    ctx.upload(S_, S)
    up_cols(cols, R_, R)
    up_cols(cols, S_, S)
    assert cols.relation_info(S_).packed == 0
    npp, stable = phj.nopart_params(), phj.radix_params((8, 8), stable=True)
    r = cols.join(npp)
    assert r.matches == ctx.join(npp).matches == O.semijoin_count(R, S)
    assert "S.pack" in timer_names(r) and "R.pack" in timer_names(r)
    assert timer_bytes(r, "S.pack") == 32 * nS
    assert cols.relation_info(S_).packed == 1 and cols.relation_info(R_).packed == 1
    r = cols.join(stable)
    assert r.matches == ctx.join(stable).matches
    assert not [n for n in timer_names(r) if n.endswith(".pack")]
    # rows: NoPartitioning keeps the probe side's input order (unique build keys: one row per probe tuple)
    assert cols.join_inner(npp).matches == ctx.join_inner(npp).matches
    assert np.array_equal(cols.joined(), ctx.joined())
    p = params()
    assert cols.join_inner(p).matches == ctx.join_inner(p).matches
    assert np.array_equal(sorted_rows(cols.joined()), sorted_rows(ctx.joined()))
    (_, nc), (_, nt) = cols.join_rows(p, phj.FULL_OUTER), ctx.join_rows(p, phj.FULL_OUTER)
    assert nc.as_dict() == nt.as_dict() and nc.probe_only > 0 and nc.build_only > 0
    assert np.array_equal(sorted_rows(cols.joined()), sorted_rows(ctx.joined()))
    (_, tc), (_, tt) = cols.join_aggregate(p, groups=True), ctx.join_aggregate(p, groups=True)
    assert tc.as_dict() == tt.as_dict()
    assert np.array_equal(sorted_rows(cols.groups()), sorted_rows(ctx.groups()))
    # the LDS join still reads the columns, and the copy stays
    r = cols.join(p)
    assert r.matches == O.semijoin_count(R, S)
    assert cols.relation_info(S_).packed == 1
    # rebinding clears it
    up_cols(cols, S_, S)
    assert cols.relation_info(S_).packed == 0


# ---- round trips and guards ----

def test_to_columns_round_trip(cols):
    n = 200_001
    cols.generate_zipf(S_, n, 1.05, 1, NR, 99)
    before = cols.download(S_)
    info = cols.relation_info(S_)
    assert (info.layout, info.owned, info.packed) == (phj.LAYOUT_TUPLES, 1, 0)
    cols.to_columns(S_)
    info = cols.relation_info(S_)
    assert (info.n, info.layout, info.has_payloads, info.owned) == (n, phj.LAYOUT_COLUMNS, 1, 1)
    assert cols.relation_ptr(S_) == (None, n)
    kp, pp, m = cols.columns_ptr(S_)
    assert m == n and kp and pp
    # each column read back as it lies in memory: bound as (n - 1) / 2 tuples of another context
    other = phj.Context(0)
    for ptr, col in ((kp, before[:, 0]), (pp, before[:, 1])):
        other.bind_device(S_, ptr, n // 2, keepalive=cols)
        assert np.array_equal(other.download(S_).reshape(-1), col[:n // 2 * 2])
    other.close()
    assert np.array_equal(cols.download(S_), before)
    assert cols.count_in_range(S_, 1, 10) == int(((before[:, 0] >= 1) & (before[:, 0] <= 10)).sum())
    cols.to_columns(S_, payloads=False)   # already columns: only the payload column goes
    assert cols.relation_info(S_).has_payloads == 0 and cols.columns_ptr(S_)[1] is None
    after = cols.download(S_)
    assert np.array_equal(after[:, 0], before[:, 0]) and not after[:, 1].any()
    cols.upload(S_, before)               # tuples replace the columns
    assert cols.relation_info(S_).layout == phj.LAYOUT_TUPLES and cols.columns_ptr(S_)[:2] == (None, None)


def test_upload_columns_round_trip(cols):
    S = half_miss(4097)
    up_cols(cols, S_, S)
    assert np.array_equal(cols.download(S_), S)
    assert cols.relation_info(S_).packed == 0


def test_group_context_refused():
    g = phj.Context(devices=[0, 0], flags=phj.CTX_LOCAL)
    try:
        with pytest.raises(phj.PhjError) as e:
            g.upload_columns(S_, np.arange(10, dtype=np.int64))
        assert e.value.code == _capi.PHJ_ERR_STATE and "single-device" in str(e.value)
        with pytest.raises(phj.PhjError) as e:
            g.relation_info(S_)
        assert "single-device" in str(e.value)
    finally:
        g.close()
