"""Host-side surface of the aggregate join (no GPU): the CLI's `--aggregate`
option and the three C ABI names in the binding's export table."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "partitionedhashjoin_amd", "phjoin")


def run(tmp_path, *args):
    return subprocess.run([CLI, "--join", "radix-partitioning", "-f", str(tmp_path / "x.txt"), *args],
                          capture_output=True, text=True, timeout=60)


def test_binding_exports_aggregate_join():
    import partitionedhashjoin_amd as phj
    from partitionedhashjoin_amd import _capi
    assert {"phj_join_aggregate", "phj_group_rows", "phj_group_download"} <= set(_capi.EXPORTED)
    assert ctypes.sizeof(_capi.JoinTotals) == 40 and ctypes.sizeof(_capi.GroupRow) == 32
    assert [f[0] for f in _capi.JoinTotals._fields_] == ["pairs", "probe_matched", "sum_a", "sum_b", "sum_ab"]
    assert [f[0] for f in _capi.GroupRow._fields_] == ["id", "payload_a", "partners", "sum_b"]
    lib = _capi.load()   # loads on a GPU-less host; the prototypes are set, no compute call is made
    P = ctypes.POINTER
    assert lib.phj_join_aggregate.argtypes == [ctypes.c_void_p, P(_capi.JoinParams), ctypes.c_uint32,
                                               P(_capi.JoinResult), P(_capi.JoinTotals)]
    assert lib.phj_join_aggregate.restype is ctypes.c_int
    assert lib.phj_group_rows.argtypes == [ctypes.c_void_p, P(ctypes.c_uint64)]
    assert lib.phj_group_rows.restype is ctypes.c_void_p
    assert lib.phj_group_download.argtypes == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
    assert (phj.AGG_GROUPS, phj.AGG_MATCHED_ONLY) == (1, 2)
    assert {"JoinTotals", "GroupRow", "AGG_GROUPS", "AGG_MATCHED_ONLY"} <= set(phj.__all__)
    assert callable(phj.Context.join_aggregate) and callable(phj.Context.groups)


def test_help_lists_aggregate_once():
    assert os.path.exists(CLI), "build first: make / __graft_entry__.build()"
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    lines = (r.stdout + r.stderr).splitlines()
    line = [ln for ln in lines if "--aggregate" in ln]
    assert len(line) == 1 and "totals" in line[0] and "groups" in line[0]
    assert len([ln for ln in lines if "--materialize" in ln]) == 1
    assert len([ln for ln in lines if "--join-kind" in ln]) == 1


def test_aggregate_rejects_unknown_value(tmp_path):
    r = run(tmp_path, "--aggregate", "sideways")
    assert r.returncode == 1
    assert "the argument ('sideways') for option '--aggregate' is invalid" in r.stdout + r.stderr


def test_aggregate_refused_with_rows_and_several_devices(tmp_path):
    for extra in (["--materialize", "all"], ["--materialize", "on"], ["--join-kind", "inner"], ["--gpus", "2"]):
        r = run(tmp_path, "--aggregate", "totals", *extra)
        assert r.returncode == 1, extra
        assert "--aggregate" in (r.stdout + r.stderr).splitlines()[0]
