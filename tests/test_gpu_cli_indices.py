"""`phjoin --rows indices` end to end on the GPU: the rows of --join-kind made
by an index join on the key columns alone (phj_join_indices) and composed with
phj_gather_column are the rows the same command makes with payloads, and those
of test_gpu_cli_outer's numpy expectation; the JSON says which way ran."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from test_gpu_cli import run_cli
from test_gpu_cli_outer import NULL, checksum

pytestmark = pytest.mark.gpu

NR, NS, SEED = 100_000, 1_500_000, 77
FIELDS = ("rows", "rows_checksum", "pairs", "probe_only", "build_only", "matches")


@functools.lru_cache(maxsize=None)
def expectation():
    """{kind: (rows, checksum, build_only)}: unique build keys 1 .. NR (payload id - 1), every probe key among them."""
    R, S = O.generate_tables(NR, NS, 1.05, SEED)
    assert np.array_equal(R[:, 1], R[:, 0] - 1) and np.all(np.isin(S[:, 0], R[:, 0]))
    lone = R[~np.isin(R[:, 0], S[:, 0])]
    assert len(lone) > 0
    anti = checksum(lone[:, 0], lone[:, 1], np.full(len(lone), NULL))
    full = (anti + checksum(S[:, 0], S[:, 0] - 1, S[:, 1])) % (1 << 64)
    return {"build-anti": (len(lone), anti, len(lone)), "full-outer": (len(lone) + NS, full, len(lone))}


@pytest.mark.parametrize("kind", ["build-anti", "full-outer"])
@pytest.mark.parametrize("join", ["radix-partitioning", "no-partitioning"])
def test_cli_rows_as_indices(tmp_path, join, kind):
    args = ("--primary", str(NR), "--secondary", str(NS), "--seed", str(SEED), "--join", join, "--join-kind", kind)
    want = run_cli(tmp_path, *args)[0]["device"]
    got = run_cli(tmp_path, *args, "--rows", "indices")[0]["device"]
    assert want["rows_as"] == "payloads" and got["rows_as"] == "indices"
    for f in FIELDS:
        assert got[f] == want[f], f
    rows, check, lone = expectation()[kind]
    assert int(got["rows"]) == int(got["matches"]) == rows
    assert int(got["rows_checksum"]) == check
    assert (int(got["pairs"]), int(got["probe_only"]), int(got["build_only"])) == (NS, 0, lone)
