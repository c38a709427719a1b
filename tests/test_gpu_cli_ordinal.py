"""`phjoin --lookup BATCHES --lookup-as codes | groups` end to end on the GPU,
against numpy over the same (seeded) relations; plain --lookup prints what it
printed before."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from test_gpu_cli import run_cli
from test_gpu_cli_lookup import N_R, N_S, SKEW, SEED, expected as expected_rows

pytestmark = pytest.mark.gpu
ARGS = ("--primary", str(N_R), "--secondary", str(N_S), "--skew", str(SKEW), "--seed", str(SEED))


@functools.lru_cache(maxsize=None)
def expected():
    R, S = O.generate_tables(N_R, N_S, SKEW, SEED)
    u, first = np.unique(R[:, 0], return_index=True)
    rank = np.empty(len(u), dtype=np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(u))
    pos = np.minimum(np.searchsorted(u, S[:, 0]), len(u) - 1)
    hit = u[pos] == S[:, 0]
    codes = np.where(hit, rank[pos], -1)
    code_sum = int((np.arange(1, N_S + 1, dtype=np.uint64) * (codes + 1).astype(np.uint64)).sum(dtype=np.uint64))
    counts = np.bincount(codes[hit], minlength=len(u)).astype(np.uint64)
    sums = np.zeros(len(u), dtype=np.uint64)
    np.add.at(sums, codes[hit], S[hit, 1].view(np.uint64))
    w = np.arange(1, len(u) + 1, dtype=np.uint64)
    return dict(found=int(hit.sum()), distinct=len(u), codes=code_sum, counts=int((w * counts).sum(dtype=np.uint64)),
                sums=int((w * sums).sum(dtype=np.uint64)))


@pytest.mark.parametrize("layout", ["tuples", "columns"])
@pytest.mark.parametrize("join", ["no-partitioning", "radix-partitioning"])
def test_cli_lookup_as_codes(tmp_path, join, layout):
    res, _ = run_cli(tmp_path, *ARGS, "--join", join, "--layout", layout, "--lookup", "4", "--lookup-as", "codes")
    dev, e = res["device"], expected()
    assert dev["lookup_as"] == "codes" and "lookup_rows_checksum" not in dev
    assert int(dev["keys_looked_up"]) == N_S and int(dev["batches"]) == 4
    assert int(dev["keys_found"]) == int(dev["matches"]) == e["found"]
    assert int(dev["index_distinct"]) == e["distinct"]
    assert int(dev["lookup_codes_checksum"]) == e["codes"]


@pytest.mark.parametrize("layout", ["tuples", "columns"])
@pytest.mark.parametrize("join", ["no-partitioning", "radix-partitioning"])
def test_cli_lookup_as_groups(tmp_path, join, layout):
    res, _ = run_cli(tmp_path, *ARGS, "--join", join, "--layout", layout, "--lookup", "4", "--lookup-as", "groups")
    dev, e = res["device"], expected()
    assert dev["lookup_as"] == "groups"
    assert int(dev["keys_looked_up"]) == N_S and int(dev["batches"]) == 4
    assert int(dev["keys_found"]) == int(dev["matches"]) == e["found"]
    assert int(dev["groups"]) == int(dev["index_distinct"]) == e["distinct"]
    assert int(dev["groups_count_checksum"]) == e["counts"]
    assert int(dev["groups_sum_checksum"]) == e["sums"]


def test_cli_plain_lookup_is_unchanged(tmp_path):
    args = (*ARGS, "--join", "no-partitioning", "--lookup", "4")
    plain, _ = run_cli(tmp_path, *args)
    rows, _ = run_cli(tmp_path, *args, "--lookup-as", "rows")
    found, checksum, distinct = expected_rows()
    for dev in (plain["device"], rows["device"]):
        assert "lookup_as" not in dev and "lookup_codes_checksum" not in dev and "groups" not in dev
        assert int(dev["lookup_rows_checksum"]) == checksum
        assert int(dev["keys_found"]) == int(dev["matches"]) == found and int(dev["index_distinct"]) == distinct
