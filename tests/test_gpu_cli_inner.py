"""`phjoin --materialize all` end to end on the GPU: Run() returns the inner
join's rows (phj_join_inner). The CLI's build side is Sequential (unique
keys), so the rows are those of `--materialize on`: one per probe tuple,
payloadA = id - 1, and the row checksum is exact."""
import json
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu
CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "partitionedhashjoin_amd", "phjoin")


@pytest.mark.parametrize("join", ["radix-partitioning", "no-partitioning"])
def test_cli_materialize_all_rows(tmp_path, join):
    nR, nS, seed = 100_000, 1_500_000, 77
    out = tmp_path / "hashjoin.txt"
    r = subprocess.run([CLI, "--log", "debug", "-f", str(out), "--primary", str(nR), "--secondary", str(nS),
                        "--seed", str(seed), "--join", join, "--materialize", "all"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(out.read_text())
    R, S = O.generate_tables(nR, nS, 1.05, seed)
    ids = S[:, 0].astype(np.uint64)
    want = int((ids * np.uint64(3) + (ids - np.uint64(1)) * np.uint64(5)
                + S[:, 1].astype(np.uint64) * np.uint64(7)).sum(dtype=np.uint64))
    assert int(res["device"]["rows"]) == int(res["device"]["matches"]) == nS
    assert int(res["device"]["rows_checksum"]) == want
