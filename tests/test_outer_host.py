"""Host-side surface of the outer and anti joins (no GPU): the CLI's
`--join-kind` option and the two C ABI names in the binding's export table."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "partitionedhashjoin_amd", "phjoin")


def run(tmp_path, *args):
    return subprocess.run([CLI, "--join", "radix-partitioning", "-f", str(tmp_path / "x.txt"), *args],
                          capture_output=True, text=True, timeout=60)


def test_help_lists_join_kinds():
    assert os.path.exists(CLI), "build first: make / __graft_entry__.build()"
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    line = [ln for ln in (r.stdout + r.stderr).splitlines() if "--join-kind" in ln]
    assert len(line) == 1 and "full-outer" in line[0]


def test_join_kind_rejects_unknown_value(tmp_path):
    r = run(tmp_path, "--join-kind", "sideways")
    assert r.returncode == 1
    assert "the argument ('sideways') for option '--join-kind' is invalid" in r.stdout + r.stderr


def test_join_kind_refused_with_materialize_and_several_devices(tmp_path):
    for extra in (["--materialize", "on"], ["--materialize", "all"], ["--gpus", "2"], ["--exchange", "local"]):
        r = run(tmp_path, "--join-kind", "inner", *extra)
        assert r.returncode == 1, extra
        assert "--join-kind" in (r.stdout + r.stderr).splitlines()[0]


def test_binding_exports_row_joins():
    import partitionedhashjoin_amd as phj
    from partitionedhashjoin_amd import _capi
    assert {"phj_join_rows_count", "phj_join_rows"} <= set(_capi.EXPORTED)
    lib = _capi.load()   # loads on a GPU-less host; the prototypes are set, no compute call is made
    assert len(lib.phj_join_rows_count.argtypes) == 5 and len(lib.phj_join_rows.argtypes) == 6
    assert lib.phj_join_rows.argtypes[3] is ctypes.c_int64
    assert ctypes.sizeof(_capi.RowCounts) == 32
    assert (phj.INNER, phj.PROBE_OUTER, phj.BUILD_OUTER, phj.FULL_OUTER, phj.PROBE_ANTI, phj.BUILD_ANTI) == \
        (1, 3, 5, 7, 2, 4)
    assert (phj.ROWS_PAIRS, phj.ROWS_PROBE_ONLY, phj.ROWS_BUILD_ONLY) == (1, 2, 4) and phj.NULL_PAYLOAD == -2**63
