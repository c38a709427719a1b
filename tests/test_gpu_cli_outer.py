"""`phjoin --join-kind` end to end on the GPU: Run() returns the rows of
phj_join_rows. The CLI's build side is Sequential (unique keys 1..|R|, payload
id - 1) and every Zipf probe key lies in [1, |R|], so each probe tuple has
exactly one pair and the build-only rows are the keys never drawn; the missing
side's payload is INT64_MIN and the row checksum wraps in uint64."""
import json
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu
CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "partitionedhashjoin_amd", "phjoin")
NULL = np.int64(-2**63).astype(np.uint64)


def checksum(ids, pa, pb):
    with np.errstate(over="ignore"):
        return int((ids.astype(np.uint64) * np.uint64(3) + pa.astype(np.uint64) * np.uint64(5)
                    + pb.astype(np.uint64) * np.uint64(7)).sum(dtype=np.uint64))


@pytest.mark.parametrize("kind", ["build-anti", "full-outer"])
@pytest.mark.parametrize("join", ["radix-partitioning", "no-partitioning"])
def test_cli_join_kind_rows(tmp_path, join, kind):
    nR, nS, seed = 100_000, 1_500_000, 77
    out = tmp_path / "hashjoin.txt"
    r = subprocess.run([CLI, "--log", "debug", "-f", str(out), "--primary", str(nR), "--secondary", str(nS),
                        "--seed", str(seed), "--join", join, "--join-kind", kind],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    dev = json.loads(out.read_text())["device"]
    R, S = O.generate_tables(nR, nS, 1.05, seed)
    assert np.array_equal(R[:, 1], R[:, 0] - 1) and np.all(np.isin(S[:, 0], R[:, 0]))
    lone = R[~np.isin(R[:, 0], S[:, 0])]
    assert len(lone) > 0
    want = checksum(lone[:, 0], lone[:, 1], np.full(len(lone), NULL))
    rows = len(lone)
    if kind == "full-outer":
        want = (want + checksum(S[:, 0], S[:, 0] - 1, S[:, 1])) % (1 << 64)
        rows += nS
    assert int(dev["pairs"]) == nS
    assert int(dev["probe_only"]) == 0
    assert int(dev["build_only"]) == len(lone)
    assert int(dev["rows"]) == int(dev["matches"]) == rows
    assert int(dev["rows_checksum"]) == want
