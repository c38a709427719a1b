"""What the row and aggregate joins report besides their rows, per entry point,
algorithm and input: the ordered list of (timer name, bytes), algorithmic_bytes,
num_partitions, matches, and the row counts or totals. The inner join, the row
joins, the index joins and the aggregates share one host driver per family;
these figures are what a caller sees of it.

The expectations (tests/golden/rows_reports.json) are what the library returned
while every family still had one driver per algorithm and the inner join a
driver of its own; print the table of the library under test with
    python tests/test_gpu_rows_reports.py > table.json

A second test pins the texts of the 2^32-row range errors and of the radix
forms' precondition.
"""
import json
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import partitionedhashjoin_amd as phj
from test_gpu_inner import R_BASE, S_BASE, dup_case, small_cases, with_payloads

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rows_reports.json")

ALGOS = {"np": phj.nopart_params, "radix": lambda: phj.radix_params((8, 8))}
INPUTS = {
    "dup": lambda: dup_case()[:2],          # duplicates across LDS rounds, unmatched tuples on both sides
    "no_pairs": lambda: small_cases()[2],   # no key in common: the zero-pairs branch
    "empty_probe": lambda: small_cases()[0],
    "empty_build": lambda: small_cases()[1],
}
CLASS_SETS = (1, 2, 3, 4, 7)


def _rows(call, classes):
    def run(c, p):
        r, n = getattr(c, call)(p, classes)
        return r, {"counts": n.as_dict()}
    return run


def _agg(**kw):
    def run(c, p):
        r, t = c.join_aggregate(p, **kw)
        return r, {"totals": t.as_dict(), "group_rows": len(c.groups())}
    return run


# entry -> (bound as key columns alone, call(ctx, params) -> (JoinResult, what else it returned))
ENTRIES = {
    "join_inner_count": (False, lambda c, p: (c.join_inner_count(p), {})),
    "join_inner": (False, lambda c, p: (c.join_inner(p), {"rows": len(c.joined())})),
    **{f"join_rows_count.{k}": (False, _rows("join_rows_count", k)) for k in CLASS_SETS},
    **{f"join_rows.{k}": (False, _rows("join_rows", k)) for k in CLASS_SETS},
    **{f"join_indices.{k}": (False, _rows("join_indices", k)) for k in (1, 7)},
    # (a key column alone: the probe reads the column itself, and the radix form's pass 1 reads less)
    **{f"join_indices.{k}.key_columns": (True, _rows("join_indices", k)) for k in (1, 7)},
    "join_aggregate.totals": (False, _agg()),
    "join_aggregate.groups": (False, _agg(groups=True)),
    "join_aggregate.groups.matched_only": (False, _agg(groups=True, matched_only=True)),
}


def reports(c, input_name, algo):
    """{entry: report} of one input under one algorithm, on context c."""
    R, S = INPUTS[input_name]()
    out = {}
    for columns in (False, True):
        if columns:
            c.upload_columns(phj.SIDE_BUILD, R[:, 0])
            c.upload_columns(phj.SIDE_PROBE, S[:, 0])
        else:
            c.upload(phj.SIDE_BUILD, R)
            c.upload(phj.SIDE_PROBE, S)
        for entry, (cols, call) in ENTRIES.items():
            if cols != columns:
                continue
            r, extra = call(c, ALGOS[algo]())
            out[entry] = {"timers": [[t[0], t[2]] for t in r.timers()], "algorithmic_bytes": r.algorithmic_bytes,
                          "num_partitions": r.num_partitions, "matches": r.matches, **extra}
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("algo", list(ALGOS))
@pytest.mark.parametrize("input_name", list(INPUTS))
def test_reports(ctx, input_name, algo):
    with open(GOLDEN) as f:
        expect = json.load(f)[input_name][algo]
    got = reports(ctx, input_name, algo)
    assert sorted(got) == sorted(expect) == sorted(ENTRIES)
    for entry in ENTRIES:
        print(f"{input_name} | {algo} | {entry}: {json.dumps(got[entry])}")
    for entry in ENTRIES:
        assert got[entry] == expect[entry], (input_name, algo, entry)


RANGE_TAIL = " rows are addressed with 32 bits (limit 2^32 - 1)"
FUSED_TAIL = " needs the fused LDS join (PHJ_FUSED, PHJ_SUBPART)"


def _refused(call, code):
    with pytest.raises(phj.PhjError) as e:
        call()
    assert e.value.code == code, str(e.value)
    head = f"phj error {code}: "
    assert str(e.value).startswith(head), str(e.value)
    return str(e.value)[len(head):]


@pytest.mark.gpu
@pytest.mark.parametrize("algo", list(ALGOS))
def test_row_range_messages(ctx, algo):
    # 65 600^2 = 4 303 360 000 pairs >= 2^32 (test_gpu_inner.test_inner_row_range_limit)
    n = 65_600
    ctx.upload(phj.SIDE_BUILD, with_payloads(np.full(n, 42), R_BASE))
    ctx.upload(phj.SIDE_PROBE, with_payloads(np.full(n, 42), S_BASE))
    p, rng = ALGOS[algo](), phj._capi.PHJ_ERR_RANGE
    assert _refused(lambda: ctx.join_inner(p), rng) == f"phj_join_inner: {n * n} pairs," + RANGE_TAIL
    assert _refused(lambda: ctx.join_rows(p, phj.INNER), rng) == f"phj_join_rows: {n * n} rows," + RANGE_TAIL
    assert _refused(lambda: ctx.join_indices(p, phj.INNER), rng).startswith("phj_join_indices: ")


@pytest.mark.gpu
def test_radix_precondition_messages(monkeypatch):
    # the radix forms run only the fused per-partition LDS join: refused without it
    R, S = small_cases()[2]
    monkeypatch.setenv("PHJ_FUSED", "0")   # read when the context is created
    p, inv = ALGOS["radix"](), phj._capi.PHJ_ERR_INVALID
    with phj.Context(0) as c:
        c.upload(phj.SIDE_BUILD, R)
        c.upload(phj.SIDE_PROBE, S)
        for call, form in ((lambda: c.join_inner_count(p), "radix inner join"),
                           (lambda: c.join_inner(p), "radix inner join"),
                           (lambda: c.join_rows_count(p, phj.FULL_OUTER), "radix row join"),
                           (lambda: c.join_rows(p, phj.FULL_OUTER), "radix row join"),
                           (lambda: c.join_indices(p, phj.FULL_OUTER), "radix row join"),
                           (lambda: c.join_aggregate(p), "radix aggregate join"),
                           (lambda: c.join_aggregate(p, groups=True), "radix aggregate join")):
            assert _refused(call, inv) == form + FUSED_TAIL


if __name__ == "__main__":
    with phj.Context(0) as c0:
        json.dump({i: {a: reports(c0, i, a) for a in ALGOS} for i in INPUTS}, sys.stdout, indent=1, sort_keys=True)
    print()
