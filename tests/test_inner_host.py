"""Host-side surface of the inner join (no GPU): the CLI's `--materialize all`
value and the two C ABI names in the binding's export table."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "partitionedhashjoin_amd", "phjoin")


def test_help_lists_materialize_all():
    assert os.path.exists(CLI), "build first: make / __graft_entry__.build()"
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    line = [ln for ln in (r.stdout + r.stderr).splitlines() if "--materialize" in ln]
    assert len(line) == 1 and "| all" in line[0]


def test_materialize_rejects_unknown_value(tmp_path):
    r = subprocess.run([CLI, "--join", "radix-partitioning", "--materialize", "maybe", "-f", str(tmp_path / "x.txt")], capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 1
    assert "is invalid" in r.stdout + r.stderr


def test_binding_exports_inner_join():
    from partitionedhashjoin_amd import _capi
    assert {"phj_join_inner_count", "phj_join_inner"} <= set(_capi.EXPORTED)
    lib = _capi.load()   # loads on a GPU-less host; the prototypes are set, no compute call is made
    assert lib.phj_join_inner.argtypes == lib.phj_join_materialize.argtypes
    assert lib.phj_join_inner_count.argtypes == lib.phj_join_materialize.argtypes
