"""Row-number joins (phj_join_indices, phj_gather_column) against numpy.

phj_join_indices is phj_join_rows returning (build row, probe row) pairs and
reading nothing but keys. The expectation never comes from the call under
test: it is test_gpu_outer.Expect (numpy) over relations whose payloads are
their row numbers plus a base, and, as a second witness, the existing join_rows
on a tuple binding whose payloads are arange, with null -1."""
import ctypes as C
import functools

import numpy as np
import pytest

import partitionedhashjoin_amd as phj
from partitionedhashjoin_amd import _capi
from test_gpu_inner import R_BASE, S_BASE, with_payloads
from test_gpu_materialize import PARAMS
from test_gpu_outer import ALL_CLASSES, NULL, Expect, few_probes_case, rounds_case, small_cases

pytestmark = pytest.mark.gpu

IDS = [p[0] for p in PARAMS]
BY_NAME = {p[0]: p for p in PARAMS}
TWO = [("np", phj.nopart_params(), True), ("radix-8+8", phj.radix_params((8, 8)), False)]
TWO_IDS = [p[0] for p in TWO]
CHUNKED = ["radix-8+8", "radix-4"]
R_, S_ = phj.SIDE_BUILD, phj.SIDE_PROBE
NO = phj.NO_ROW


def canon2(b, p):
    """(build row, probe row) pairs in a canonical order."""
    a = np.stack([np.asarray(b, dtype=np.int64), np.asarray(p, dtype=np.int64)], axis=1)
    return a[np.lexsort((a[:, 0], a[:, 1]))]


_want = {}


def want_pairs(E, classes):
    """E.rows(classes) as index pairs: payload - base, NULL -> NO_ROW."""
    key = (id(E), classes)
    if key not in _want:
        rows = E.rows(classes)
        b = np.where(rows[:, 1] == NULL, NO, rows[:, 1] - R_BASE)
        p = np.where(rows[:, 2] == NULL, NO, rows[:, 2] - S_BASE)
        out = canon2(b, p)
        out.setflags(write=False)
        _want[key] = (E, out)   # (E kept alive: its id is the key)
    return _want[key][1]


def bind_keys(c, E):
    """Both sides as key columns alone."""
    c.upload_columns(R_, E.R[:, 0])
    c.upload_columns(S_, E.S[:, 0])


def timer_names(r):
    return [t[0] for t in r.timers()]


def timer_bytes(r):
    return {t[0]: t[2] for t in r.timers()}


def check_idx(c, params, ordered, E, classes, bind=True):
    """join_indices of one class set against E; returns (build_rows, probe_rows)."""
    if bind:
        bind_keys(c, E)
    want = E.counts(classes)
    r, n = c.join_indices(params, classes)
    assert (n.pairs, n.probe_only, n.build_only, n.rows) == want and r.matches == want[3]
    b, p = c.joined_indices()
    assert len(b) == len(p) == want[3] == c.joined_indices_ptr()[2]
    assert np.array_equal(canon2(b, p), want_pairs(E, classes))
    # the probe part: every probe tuple's rows contiguous, NoPartitioning in
    # input order; then the build-only rows
    nprobe = want[3] - want[2]
    pp = p[:nprobe]
    assert np.all(pp != NO)
    assert (1 + int(np.count_nonzero(pp[1:] != pp[:-1])) if nprobe else 0) == len(np.unique(pp))
    if ordered:
        assert np.all(pp[1:] >= pp[:-1])
    assert np.all(p[nprobe:] == NO) and np.all(b[nprobe:] != NO)
    assert not [t for t in timer_names(r) if t.endswith(".pack")]
    return b, p


# ---- all seven class sets, key columns alone ----

@pytest.mark.parametrize("classes", ALL_CLASSES)
@pytest.mark.parametrize("name,params,ordered", PARAMS, ids=IDS)
def test_indices_all_class_sets(ctx, name, params, ordered, classes):
    for E in (rounds_case(), few_probes_case()):
        check_idx(ctx, params, ordered, E, classes)
        assert ctx.relation_info(R_).packed == 0 and ctx.relation_info(S_).packed == 0


# ---- no pack; pass 1 is accounted 8 B per tuple less ----

@pytest.mark.parametrize("name,params,ordered", PARAMS, ids=IDS)
def test_indices_no_pack_and_bytes(ctx, name, params, ordered):
    E = rounds_case()
    ctx.upload(R_, E.R)
    ctx.upload(S_, E.S)
    rt, _ = ctx.join_rows(params, phj.FULL_OUTER)
    tb = timer_bytes(rt)
    bind_keys(ctx, E)
    ri, _ = ctx.join_indices(params, phj.FULL_OUTER)
    ib = timer_bytes(ri)
    for side in (R_, S_):
        info = ctx.relation_info(side)
        assert (info.layout, info.has_payloads, info.packed) == (phj.LAYOUT_COLUMNS, 0, 0)
    assert not [t for t in ib if t.endswith(".pack")], list(ib)
    sides = [("R", len(E.R))] + ([] if name.startswith("np") else [("S", len(E.S))])
    for tag, n in sides:
        for t in (tag + ".p1.hist", tag + ".p1.scatter"):
            assert ib[t] == tb[t] - 8 * n, (t, ib[t], tb[t])
    if name.startswith("np"):
        assert not [t for t in ib if t.startswith("S.p")]
    for t in ("rows.count", "rows.emit", "rows.build_only"):
        assert t in ib
    # 16 B per row written where the row join writes 24
    assert tb["rows.build_only"] - ib["rows.build_only"] == 8 * len(E.build_rows)
    assert ri.algorithmic_bytes < rt.algorithmic_bytes


# ---- the binding does not matter; join_rows on arange payloads agrees ----

@pytest.mark.parametrize("name,params,ordered", TWO, ids=TWO_IDS)
def test_indices_any_binding(ctx, name, params, ordered):
    E = few_probes_case()
    rng = np.random.default_rng(99)
    junk_r, junk_s = rng.integers(-2**62, 2**62, len(E.R)), rng.integers(-2**62, 2**62, len(E.S))
    want = want_pairs(E, phj.FULL_OUTER)

    def once():
        before = [ctx.relation_info(s).as_dict() for s in (R_, S_)]
        b, p = check_idx(ctx, params, ordered, E, phj.FULL_OUTER, bind=False)
        assert [ctx.relation_info(s).as_dict() for s in (R_, S_)] == before
        return b, p

    ctx.upload(R_, np.stack([E.R[:, 0], junk_r], axis=1))          # tuples, garbage payloads
    ctx.upload(S_, np.stack([E.S[:, 0], junk_s], axis=1))
    once()
    ctx.upload_columns(R_, E.R[:, 0], junk_r)                      # columns, garbage payloads
    ctx.upload_columns(S_, E.S[:, 0], junk_s)
    once()
    assert ctx.relation_info(S_).has_payloads == 1
    bind_keys(ctx, E)                                              # key columns alone
    once()
    ctx.upload(R_, E.R)                                            # one side each way
    once()
    # the second witness: the row join on tuples whose payloads are arange
    ctx.upload(R_, with_payloads(E.R[:, 0], 0))
    ctx.upload(S_, with_payloads(E.S[:, 0], 0))
    ctx.join_rows(params, phj.FULL_OUTER, NO)
    rows = ctx.joined()
    assert np.array_equal(canon2(rows[:, 1], rows[:, 2]), want)


# ---- tile and column edges ----

@functools.lru_cache(maxsize=None)
def half_missing(ns):
    """ns probe tuples against 1000 unique build keys, every other one missing."""
    rng = np.random.default_rng(1000 + ns)
    sk = rng.integers(1, 1001, ns)
    sk[::2] += 5000
    return Expect(with_payloads(np.arange(1, 1001), R_BASE), with_payloads(sk, S_BASE))


@functools.lru_cache(maxsize=None)
def small_build(nr):
    """nr unique build keys against 20 011 probe tuples, about half of them missing."""
    sk = np.random.default_rng(2000 + nr).integers(1, 2 * nr + 1, 20_011)
    return Expect(with_payloads(np.arange(1, nr + 1), R_BASE), with_payloads(sk, S_BASE))


def check_edges(ctx, params, ordered, E):
    b, p = check_idx(ctx, params, ordered, E, phj.FULL_OUTER)
    for col, n in ((b, len(E.R)), (p, len(E.S))):   # the first and the last row number of each side
        assert np.any(col == 0) and np.any(col == n - 1) and col.max() == n - 1 and col.min() >= NO


@pytest.mark.parametrize("ns", [1, 63, 64, 4095, 4096, 4097, 8193, 3 * 4096 + 5])
@pytest.mark.parametrize("name,params,ordered", TWO, ids=TWO_IDS)
def test_indices_probe_edges(ctx, name, params, ordered, ns):
    check_edges(ctx, params, ordered, half_missing(ns))


@pytest.mark.parametrize("nr", [1, 257, 4097])
@pytest.mark.parametrize("name,params,ordered", TWO, ids=TWO_IDS)
def test_indices_build_edges(ctx, name, params, ordered, nr):
    check_edges(ctx, params, ordered, small_build(nr))


# ---- the chunked pass 1 ----

@pytest.mark.parametrize("classes", [phj.FULL_OUTER, phj.INNER])
@pytest.mark.parametrize("name", CHUNKED)
def test_indices_chunked_pass1(chunk_ctx, name, classes):
    _, params, ordered = BY_NAME[name]
    E = rounds_case()
    check_idx(chunk_ctx, params, ordered, E, classes)                  # key columns
    chunk_ctx.upload(R_, E.R)                                          # tuples, payloads ignored
    chunk_ctx.upload(S_, E.S)
    check_idx(chunk_ctx, params, ordered, E, classes, bind=False)


# ---- nothing but the keys is read; an 8-byte aligned base works ----

GUARD = 4099   # odd (the bound base is 8-B but not 16-B aligned) and more than a tile


@pytest.mark.parametrize("name,params,ordered", TWO, ids=TWO_IDS)
def test_indices_guarded_columns(ctx, name, params, ordered):
    E = rounds_case()
    guard = np.full(GUARD, 7, dtype=np.int64)      # a key both sides hold: an over-read changes the pair count
    donors = []
    for side, rel in ((R_, E.R), (S_, E.S)):
        d = phj.Context(0)
        d.upload_columns(S_, np.concatenate([guard, rel[:, 0], guard]))
        base = d.columns_ptr(S_)[0]
        assert base % 16 == 0 and (base + 8 * GUARD) % 16 == 8
        ctx.bind_columns(side, base + 8 * GUARD, None, len(rel), keepalive=d)
        donors.append(d)
    try:
        for classes in (phj.FULL_OUTER, phj.INNER):
            check_idx(ctx, params, ordered, E, classes, bind=False)
    finally:
        bind_keys(ctx, small_cases()[2])   # (rebinding releases the donors)
        for d in donors:
            d.close()


@pytest.mark.parametrize("name,params,ordered", TWO, ids=TWO_IDS)
def test_indices_stride_trap(ctx, name, params, ordered):
    E = rounds_case()
    donors = []
    for side, rel in ((R_, E.R), (S_, E.S)):
        trap = np.full(len(rel), 7, dtype=np.int64)   # what a 16-B stride would read from buf[n:2n]: all match
        d = phj.Context(0)
        d.upload_columns(S_, np.concatenate([rel[:, 0], trap]))
        ctx.bind_columns(side, d.columns_ptr(S_)[0], None, len(rel), keepalive=d)
        donors.append(d)
    try:
        check_idx(ctx, params, ordered, E, phj.FULL_OUTER, bind=False)
    finally:
        bind_keys(ctx, small_cases()[2])
        for d in donors:
            d.close()


# ---- one result at a time ----

@pytest.mark.parametrize("name,params,ordered", TWO, ids=TWO_IDS)
def test_indices_and_rows_replace_each_other(ctx, name, params, ordered):
    E = few_probes_case()
    ctx.upload(R_, E.R)
    ctx.upload(S_, E.S)
    ctx.join_rows(params, phj.FULL_OUTER)
    kept = ctx.joined()
    assert len(kept) == E.counts(phj.FULL_OUTER)[3] and ctx.joined_indices_ptr() == (None, None, 0)
    b, p = check_idx(ctx, params, ordered, E, phj.FULL_OUTER, bind=False)
    assert ctx.joined().shape == (0, 3)
    # the counting calls and the aggregate disturb neither
    ctx.join_rows_count(params, phj.BUILD_ANTI)
    ctx.join_inner_count(params)
    ctx.join_aggregate(params, groups=True)
    b2, p2 = ctx.joined_indices()
    assert np.array_equal(b2, b) and np.array_equal(p2, p) and ctx.joined().shape == (0, 3)
    for call in (lambda: ctx.join_rows(params, phj.PROBE_OUTER), lambda: ctx.join_inner(params),
                 lambda: ctx.join_materialize(params)):
        check_idx(ctx, params, ordered, E, phj.BUILD_OUTER, bind=False)
        assert ctx.joined_indices_ptr()[2] > 0
        call()
        assert ctx.joined_indices_ptr() == (None, None, 0)
        assert [len(a) for a in ctx.joined_indices()] == [0, 0] and len(ctx.joined()) > 0


# ---- poisoned workspace ----

@pytest.mark.parametrize("name,params,ordered", TWO, ids=TWO_IDS)
def test_indices_poisoned_workspace(name, params, ordered):
    with phj.Context(0) as fresh:
        fresh.debug_poison_alloc(0xFF)
        check_idx(fresh, params, ordered, rounds_case(), phj.FULL_OUTER)


# ---- limits and refusals ----

@pytest.mark.parametrize("name,params,ordered", TWO, ids=TWO_IDS)
def test_indices_range_limit(ctx, name, params, ordered):
    # 65 600^2 = 4 303 360 000 pairs >= 2^32: counted exactly, not materialised
    n = 65_600
    ctx.upload_columns(R_, np.full(n, 42))
    ctx.upload_columns(S_, np.full(n, 42))
    r, c = _capi.JoinResult(), _capi.RowCounts()
    rc = ctx._L.phj_join_indices(ctx._h, C.byref(params), phj.FULL_OUTER, C.byref(r), C.byref(c))
    assert rc == _capi.PHJ_ERR_RANGE
    assert (c.pairs, c.probe_only, c.build_only, c.rows) == (n * n, 0, 0, n * n) and r.matches == n * n
    assert ctx.joined_indices_ptr() == (None, None, 0)
    with pytest.raises(phj.PhjError) as e:
        ctx.join_indices(params, phj.INNER)
    assert e.value.code == _capi.PHJ_ERR_RANGE and "phj_join_indices" in str(e.value)
    r, c = ctx.join_indices(params, phj.ROWS_PROBE_ONLY | phj.ROWS_BUILD_ONLY)   # no pair rows asked: no limit met
    assert (c.pairs, c.probe_only, c.build_only, c.rows) == (n * n, 0, 0, 0)
    check_idx(ctx, params, ordered, small_cases()[2], phj.FULL_OUTER)   # a small join afterwards is exact


@pytest.mark.parametrize("classes", [0, 8, 9, 1 << 31])
def test_indices_bad_classes_refused(ctx, classes):
    bind_keys(ctx, small_cases()[2])
    for p in (phj.nopart_params(), phj.radix_params((8, 8))):
        with pytest.raises(phj.PhjError) as e:
            ctx.join_indices(p, classes)
        assert e.value.code == _capi.PHJ_ERR_INVALID


def test_indices_group_context_refused():
    with phj.Context(devices=[0, 0], flags=phj.CTX_LOCAL) as g:
        with pytest.raises(phj.PhjError, match="single-device") as e:
            g.join_indices(phj.radix_params((8, 8)), phj.FULL_OUTER)
        assert e.value.code == _capi.PHJ_ERR_STATE
        with pytest.raises(phj.PhjError) as e:
            g.gather_column(0, 0, 0, 1, 0, 0)
        assert e.value.code == _capi.PHJ_ERR_STATE


@pytest.mark.parametrize("name,params,ordered", TWO, ids=TWO_IDS)
def test_indices_empty_and_tiny_sides(ctx, name, params, ordered):
    for E in small_cases():
        for classes in ALL_CLASSES:
            b, p = check_idx(ctx, params, ordered, E, classes)
            if len(E.R) == 0 or len(E.S) == 0:   # no join ran: the other side's row numbers in input order
                ns = len(E.S) if classes & phj.ROWS_PROBE_ONLY else 0
                nr = len(E.R) if classes & phj.ROWS_BUILD_ONLY else 0
                assert np.array_equal(p, np.concatenate([np.arange(ns), np.full(nr, NO)]))
                assert np.array_equal(b, np.concatenate([np.full(ns, NO), np.arange(nr)]))


# ---- the gather ----

class DeviceColumn:
    """An int64 column in device memory: the key column of a donor context."""

    def __init__(self, values):
        self.ctx = phj.Context(0)
        self.n = len(values)
        self.ctx.upload_columns(S_, np.asarray(values, dtype=np.int64))
        self.ptr = self.ctx.columns_ptr(S_)[0]

    def read(self):
        return self.ctx.download(S_)[:, 0]

    def close(self):
        self.ctx.close()


@pytest.fixture()
def columns():
    made = []

    def make(values):
        made.append(DeviceColumn(values))
        return made[-1]

    yield make
    for d in made:
        d.close()


def gather_expect(src, idx, null, out):
    idx = np.asarray(idx)
    ok = (idx >= 0) & (idx < len(src))
    want = np.array(out, dtype=np.int64)
    want[ok] = np.asarray(src)[idx[ok]]
    if null is not None:
        want[~ok] = null
    return want


@pytest.mark.parametrize("name,params,ordered", TWO, ids=TWO_IDS)
def test_gather_composes_the_row_join(ctx, columns, name, params, ordered):
    E = few_probes_case()
    b, p = check_idx(ctx, params, ordered, E, phj.FULL_OUTER)
    bp, pp, n = ctx.joined_indices_ptr()
    assert n == len(b) and bp and pp
    rk, rpay, sk, spay = (columns(a) for a in (E.R[:, 0], E.R[:, 1], E.S[:, 0], E.S[:, 1]))
    ident, pa, pb = (columns(np.full(n, 123_456_789)) for _ in range(3))
    ctx.gather_column(spay.ptr, spay.n, pp, n, NULL, pb.ptr)
    assert np.array_equal(pb.read(), gather_expect(E.S[:, 1], p, NULL, np.zeros(n)))
    ctx.gather_column(rpay.ptr, rpay.n, bp, n, NULL, pa.ptr)
    # the id: the probe key, then the build key where there is a build row (null_value None keeps the rest)
    ctx.gather_column(sk.ptr, sk.n, pp, n, 0, ident.ptr)
    ctx.gather_column(rk.ptr, rk.n, bp, n, None, ident.ptr)
    got = np.stack([ident.read(), pa.read(), pb.read()], axis=1)
    ctx.upload(R_, E.R)
    ctx.upload(S_, E.S)
    ctx.join_rows(params, phj.FULL_OUTER, NULL)
    rows = ctx.joined()
    order = lambda a: a[np.lexsort((a[:, 0], a[:, 1], a[:, 2]))]
    assert np.array_equal(order(got), order(rows))
    assert np.array_equal(order(got), order(E.rows(phj.FULL_OUTER)))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_gather_sizes(ctx, columns, n):
    rng = np.random.default_rng(n)
    src = rng.integers(-2**62, 2**62, 1001)
    idx = rng.integers(-1, 1001, n)
    if n:
        idx[0], idx[-1] = 1000, 0
    s, i, o = columns(src), columns(idx if n else [0]), columns(np.full(max(n, 1), 5))
    ctx.gather_column(s.ptr, len(src), i.ptr, n, -77, o.ptr)
    assert np.array_equal(o.read()[:n], gather_expect(src, idx, -77, np.full(n, 5)))
    assert np.array_equal(o.read()[n:], np.full(max(n, 1) - n, 5))   # nothing behind n is written
    ctx.gather_column(s.ptr, len(src), i.ptr, n, None, o.ptr)
    assert np.array_equal(o.read()[:n], gather_expect(src, idx, -77, np.full(n, 5)))


def test_gather_bad_indices(ctx, columns):
    src = np.arange(100, 200)
    idx = np.tile(np.array([3, 99, NO, 0]), 40)
    bad = {5: len(src), 70: -2, 131: 2**40}
    for at, v in bad.items():
        idx[at] = v
    s, i, o = columns(src), columns(idx), columns(np.full(len(idx), 9))
    for null, keep in ((-5, None), (None, 9)):
        with pytest.raises(phj.PhjError) as e:
            ctx.gather_column(s.ptr, len(src), i.ptr, len(idx), null, o.ptr)
        assert e.value.code == _capi.PHJ_ERR_RANGE and "3 indices" in str(e.value)
        got = o.read()
        want = gather_expect(src, idx, null, np.full(len(idx), 9))
        assert np.array_equal(got, want)
        for at in bad:   # the null treatment, and right neighbours
            assert got[at] == (null if null is not None else keep)
            assert got[at - 1] == want[at - 1] and got[at + 1] == want[at + 1]
        i2 = columns(np.full(len(idx), 10**6))     # a whole column of bad indices
        with pytest.raises(phj.PhjError, match=f"{len(idx)} indices"):
            ctx.gather_column(s.ptr, len(src), i2.ptr, len(idx), null, o.ptr)
        o.ctx.upload_columns(S_, np.full(len(idx), 9))
        o.ptr = o.ctx.columns_ptr(S_)[0]


def test_joined_indices_to(ctx, columns):
    E = few_probes_case()
    b, p = check_idx(ctx, TWO[1][1], False, E, phj.FULL_OUTER)
    n = len(b)
    db, dp = columns(np.zeros(n)), columns(np.zeros(n))
    ctx.joined_indices_to(db.ptr, dp.ptr, n)
    assert np.array_equal(db.read(), b) and np.array_equal(dp.read(), p)
    half = n // 2
    dq = columns(np.full(n, -9))
    ctx.joined_indices_to(None, dq.ptr, half)       # one column, a prefix
    assert np.array_equal(dq.read(), np.concatenate([p[:half], np.full(n - half, -9)]))
    with pytest.raises(phj.PhjError) as e:
        ctx.joined_indices_to(db.ptr, None, n + 1)
    assert e.value.code == _capi.PHJ_ERR_RANGE
