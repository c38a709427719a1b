"""`phjoin --lookup BATCHES` end to end on the GPU: the keys found equal the
count join's matches on the same arguments, and the rows' checksum numpy's
over the same (seeded) relations."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from test_gpu_cli import run_cli

pytestmark = pytest.mark.gpu

N_R, N_S, SKEW, SEED = 30_000, 250_001, 1.05, 515


@functools.lru_cache(maxsize=None)
def expected():
    R, S = O.generate_tables(N_R, N_S, SKEW, SEED)   # the CLI's host generator == the oracle's
    S = S.copy()
    u, first = np.unique(R[:, 0], return_index=True)
    pos = np.minimum(np.searchsorted(u, S[:, 0]), len(u) - 1)
    rows = np.where(u[pos] == S[:, 0], first[pos], -1)
    checksum = int((np.arange(1, N_S + 1, dtype=np.uint64) * (rows + 1).astype(np.uint64)).sum(dtype=np.uint64))
    return int((rows >= 0).sum()), checksum, len(u)


@pytest.mark.parametrize("layout", ["tuples", "columns"])
@pytest.mark.parametrize("join", ["no-partitioning", "radix-partitioning"])
def test_cli_lookup_equals_the_count_join(tmp_path, join, layout):
    args = ("--primary", str(N_R), "--secondary", str(N_S), "--skew", str(SKEW), "--seed", str(SEED),
            "--join", join, "--layout", layout)
    res, log = run_cli(tmp_path, *args, "--lookup", "4")
    count, _ = run_cli(tmp_path, *args)
    found, checksum, distinct = expected()
    dev = res["device"]
    assert int(dev["keys_looked_up"]) == N_S and int(dev["batches"]) == 4
    assert int(dev["keys_found"]) == int(dev["matches"]) == int(count["device"]["matches"]) == found
    assert int(dev["lookup_rows_checksum"]) == checksum
    assert int(dev["index_rows"]) == N_R and int(dev["index_distinct"]) == distinct
    assert int(dev["index_build_us"]) >= 0 and int(dev["lookup_batch_us"]) >= 0
    assert dev["layout"] == layout
    assert "Joined" in log and str(found) in log


def test_cli_lookup_more_batches_than_keys(tmp_path):
    res, _ = run_cli(tmp_path, "--primary", "50", "--secondary", "7", "--seed", "3", "--join", "no-partitioning",
                     "--lookup", "16")
    dev = res["device"]
    assert int(dev["keys_looked_up"]) == 7 and int(dev["keys_found"]) == int(dev["matches"]) == 7
