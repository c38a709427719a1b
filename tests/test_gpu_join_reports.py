"""What phj_join_materialize, phj_join_inner_count and phj_join_inner report
besides the rows: the names of their timers, the bytes of the join timers and
algorithmic_bytes, for the radix and the NoPartitioning form, and the radix
forms' precondition messages. The expectations restate the host code's
formulas (phj_capi.hip: partition_bytes, inner_count_bytes, rows_emit_bytes
with its pair pass, and the sums form_setup and rows_passes make of them) in
Python."""
import math

import pytest

import partitionedhashjoin_amd as phj
from test_gpu_inner import dup_case

pytestmark = pytest.mark.gpu

PASS = ["hist", "scan", "scatter"]


def np_buckets(n_build, ratio=2.0, slots=7, region=1024):
    """Buckets of the NoPartitioning table (np_build): regions of at most 1024."""
    nb0 = max(1, math.ceil(n_build * ratio / slots))
    rbits = min(22, max(1, ((nb0 + region - 1) // region - 1).bit_length()))
    return ((nb0 + (1 << rbits) - 1) >> rbits) << rbits, rbits


def partition_bytes(npass, n):
    return n * (16 + 32) + (n * (8 + 32) if npass == 2 else 0)


def inner_count_bytes(n_r, n_s):
    return n_r * 8 + n_s * (8 + 4)


def inner_emit_bytes(n_r, n_s, rows):
    return n_s * 12 + n_r * 8 + n_s * (16 + 4) + rows * (8 + 24)


def expected(algo, call, n_r, n_s, semi, pairs):
    """(timer names, {join timer: bytes}, algorithmic_bytes)."""
    if algo == "radix":   # 8 + 8 bits: two passes over both sides, tile kernels
        names = {f"{s}.{p}.{k}" for s in "RS" for p in ("p1", "p2") for k in PASS}
        part = partition_bytes(2, n_r) + partition_bytes(2, n_s)
        if call == "join_materialize":
            join = {"mat.join": n_r * 8 + n_s * 12, "mat.write": n_s * 20 + n_s * 4}
            return names | set(join), join, part + n_r * 8 + n_s * 12 + semi * 24
        join = {"inner.count": inner_count_bytes(n_r, n_s)}
        total = part + inner_count_bytes(n_r, n_s)
        if call == "join_inner":
            join["inner.emit"] = inner_emit_bytes(n_r, n_s, pairs)
            total += inner_emit_bytes(n_r, n_s, pairs)
        return names | set(join), join, total
    nb, rbits = np_buckets(n_r)
    assert rbits <= 8   # the build side is partitioned into the regions in one pass
    table = nb * 64
    names = {f"R.p1.{k}" for k in PASS} | {"np.build"}
    if call == "join_materialize":
        join = {"np.probe": n_s * 16 + table, "mat.write": n_s * 20 + n_s * 4}
        return names | set(join), join, n_r * 32 + n_s * 16 + table + semi * 24
    join = {"inner.count": inner_count_bytes(0, n_s) + table}
    total = n_r * 32 + table + inner_count_bytes(0, n_s) + table
    if call == "join_inner":
        join["inner.emit"] = inner_emit_bytes(0, n_s, pairs) + table
        total += inner_emit_bytes(0, n_s, pairs) + table
    return names | set(join), join, total


CASES = [("radix", phj.radix_params((8, 8))), ("np", phj.nopart_params())]


@pytest.mark.parametrize("algo,params", CASES, ids=[c[0] for c in CASES])
def test_timer_names_and_bytes(ctx, algo, params):
    R, S, pairs, _, semi = dup_case()
    ctx.upload(phj.SIDE_BUILD, R)
    ctx.upload(phj.SIDE_PROBE, S)
    for call, matches in (("join_materialize", semi), ("join_inner_count", pairs), ("join_inner", pairs)):
        r = getattr(ctx, call)(params)
        assert r.matches == matches, call
        names, join, total = expected(algo, call, len(R), len(S), semi, pairs)
        timers = r.timers()
        print(call, algo, r.algorithmic_bytes, total, sorted(t[0] for t in timers))
        assert len(timers) == len(names), call
        assert {t[0] for t in timers} == names, call
        got = {t[0]: t[2] for t in timers}
        assert {k: got[k] for k in join} == join, call
        assert r.algorithmic_bytes == total, call
        assert r.num_partitions == (1 << 16 if algo == "radix" else 0), call


def test_radix_precondition_messages(monkeypatch):
    # the radix forms run only the fused per-partition LDS join: refused without it
    R, S = dup_case()[:2]
    monkeypatch.setenv("PHJ_FUSED", "0")   # read when the context is created
    with phj.Context(0) as c:
        c.upload(phj.SIDE_BUILD, R)
        c.upload(phj.SIDE_PROBE, S)
        for call, start in ((c.join_materialize, "materialised radix join needs"),
                            (c.join_inner_count, "radix inner join needs"),
                            (c.join_inner, "radix inner join needs")):
            with pytest.raises(phj.PhjError) as e:
                call(phj.radix_params((8, 8)))
            assert e.value.code == phj._capi.PHJ_ERR_INVALID
            assert str(e.value).startswith(f"phj error {phj._capi.PHJ_ERR_INVALID}: {start}"), str(e.value)
