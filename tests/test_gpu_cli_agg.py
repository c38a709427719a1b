"""`phjoin --aggregate totals|groups` end to end on the GPU: the reported
aggregates equal the Python binding's on the same (seeded) relations."""
import functools

import numpy as np
import pytest

import partitionedhashjoin_amd as phj
from oracle import oracle as O
from test_gpu_cli import run_cli

pytestmark = pytest.mark.gpu

N_R, N_S, SKEW, SEED = 30_000, 250_000, 1.05, 515
JOINS = {"radix-partitioning": phj.radix_params(num_partitions=32, hash=phj.HASH_XXH3),
         "no-partitioning": phj.nopart_params()}
M64 = (1 << 64) - 1


@functools.lru_cache(maxsize=None)
def tables():
    return O.generate_tables(N_R, N_S, SKEW, SEED)   # the CLI's host generator == the oracle's


def checksum(rows):
    u = rows.view(np.uint64)
    w = np.array([3, 5, 7, 11], dtype=np.uint64)
    return int((u * w).sum(dtype=np.uint64))


@pytest.mark.parametrize("what", ["totals", "groups"])
@pytest.mark.parametrize("join", list(JOINS))
def test_cli_aggregate_equals_binding(ctx, tmp_path, join, what):
    res, _ = run_cli(tmp_path, "--primary", str(N_R), "--secondary", str(N_S), "--skew", str(SKEW),
                     "--seed", str(SEED), "--join", join, "--aggregate", what)
    R, S = tables()
    ctx.upload(phj.SIDE_BUILD, R)
    ctx.upload(phj.SIDE_PROBE, S)
    r, t = ctx.join_aggregate(JOINS[join], groups=what == "groups")
    dev = res["device"]
    assert int(dev["matches"]) == int(dev["pairs"]) == t.pairs == N_S
    assert int(dev["probe_matched"]) == t.probe_matched
    assert (int(dev["sum_a"]), int(dev["sum_b"]), int(dev["sum_ab"])) == (t.sum_a, t.sum_b, t.sum_ab)
    if what == "groups":
        rows = ctx.groups()
        assert int(dev["groups"]) == len(rows) == N_R
        assert int(dev["groups_checksum"]) == checksum(rows)
    else:
        assert "groups" not in dev and "groups_checksum" not in dev
