"""`phjoin --member probe|build|both` end to end on the GPU: the reported
counts and mask checksums equal numpy's over the same (seeded) relations."""
import functools
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from test_gpu_cli import CLI, run_cli

pytestmark = pytest.mark.gpu

N_R, N_S, SKEW, SEED = 30_000, 250_000, 1.05, 515


@functools.lru_cache(maxsize=None)
def expected():
    R, S = O.generate_tables(N_R, N_S, SKEW, SEED)   # the CLI's host generator == the oracle's
    ps, pr = np.isin(S[:, 0], R[:, 0]), np.isin(R[:, 0], S[:, 0])
    return ps, pr


def checksum(mask):
    """Σ (i + 1) · mask[i] mod 2^64"""
    return int((np.arange(1, len(mask) + 1, dtype=np.uint64) * mask.astype(np.uint64)).sum(dtype=np.uint64))


@pytest.mark.parametrize("layout", ["tuples", "columns"])
@pytest.mark.parametrize("join", ["no-partitioning", "radix-partitioning"])
def test_cli_member_both_equals_numpy(tmp_path, join, layout):
    res, _ = run_cli(tmp_path, "--primary", str(N_R), "--secondary", str(N_S), "--skew", str(SKEW),
                     "--seed", str(SEED), "--join", join, "--member", "both", "--layout", layout)
    ps, pr = expected()
    assert 0 < pr.sum() < N_R                       # some build rows have no partner: the build mask says which
    dev = res["device"]
    assert int(dev["matches"]) == int(dev["probe_matched"]) == int(ps.sum()) == N_S
    assert int(dev["build_matched"]) == int(pr.sum())
    assert int(dev["probe_mask_checksum"]) == checksum(ps)
    assert int(dev["build_mask_checksum"]) == checksum(pr)
    assert dev["layout"] == layout


def test_cli_member_probe_alone(tmp_path):
    res, _ = run_cli(tmp_path, "--primary", str(N_R), "--secondary", str(N_S), "--skew", str(SKEW),
                     "--seed", str(SEED), "--join", "no-partitioning", "--member", "probe")
    ps, _ = expected()
    dev = res["device"]
    assert int(dev["probe_matched"]) == int(ps.sum()) and int(dev["build_matched"]) == 0
    assert int(dev["probe_mask_checksum"]) == checksum(ps) and "build_mask_checksum" not in dev


@pytest.mark.parametrize("extra,first", [
    (["--materialize", "on"], "--member returns no rows"), (["--materialize", "all"], "--member returns no rows"),
    (["--join-kind", "full-outer"], "--member returns no rows"), (["--aggregate", "groups"], "--member returns no rows"),
    (["--rows", "indices", "--join-kind", "inner"], "--member returns no rows"),
    (["--gpus", "2"], "--member runs on one device"), (["--exchange", "local"], "--member runs on one device"),
])
def test_cli_member_exclusive_options(tmp_path, extra, first):
    r = subprocess.run([CLI, "--join", "no-partitioning", "-f", str(tmp_path / "x.txt"), "--member", "both", *extra],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1
    assert r.stdout.splitlines()[0].startswith(first), r.stdout[:300]
