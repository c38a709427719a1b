"""Row-number joins: what can be checked without a GPU. The four C ABI symbols
are in the header, the binding's export table and the library; every new call
refuses a null context before touching a device; the Python names exist; the
CLI knows --rows and refuses it where it has no rows to make."""
import ctypes as C
import os
import subprocess

import partitionedhashjoin_amd as phj
from partitionedhashjoin_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "partitionedhashjoin_amd", "phjoin")
NEW = ["phj_join_indices", "phj_joined_indices", "phj_joined_indices_download", "phj_gather_column"]


def run(tmp_path, *args):
    return subprocess.run([CLI, "--join", "radix-partitioning", "-f", str(tmp_path / "x.txt"), *args],
                          capture_output=True, text=True, timeout=60)


def test_symbols_exported_and_listed():
    L = _capi.load()
    header = open(os.path.join(ROOT, "include", "phj.h")).read()
    for name in NEW:
        assert name in _capi.EXPORTED
        assert hasattr(L, name)
        assert f"int {name}(phj_ctx *ctx" in header
    assert "#define PHJ_NO_ROW (-1)" in header
    assert "#define PHJ_ABI_VERSION 2" in header
    assert "replaces nothing in the reference" in header.lower()
    assert _capi.NO_ROW == -1 and _capi.ABI_VERSION == 2


def test_prototypes():
    L = _capi.load()
    assert len(L.phj_join_indices.argtypes) == 5       # no null payload: the marker is PHJ_NO_ROW
    assert len(L.phj_joined_indices.argtypes) == 4
    assert len(L.phj_joined_indices_download.argtypes) == 4
    assert len(L.phj_gather_column.argtypes) == 7


def test_null_context_is_invalid():
    L = _capi.load()
    r, n = _capi.JoinResult(), _capi.RowCounts()
    p = phj.radix_params((8, 8))
    b, q, m = C.c_void_p(), C.c_void_p(), C.c_uint64()
    null = C.c_int64(0)
    assert L.phj_join_indices(None, C.byref(p), phj.FULL_OUTER, C.byref(r), C.byref(n)) == _capi.PHJ_ERR_INVALID
    assert L.phj_joined_indices(None, C.byref(b), C.byref(q), C.byref(m)) == _capi.PHJ_ERR_INVALID
    assert L.phj_joined_indices_download(None, None, None, 0) == _capi.PHJ_ERR_INVALID
    assert L.phj_gather_column(None, None, 0, None, 0, C.byref(null), None) == _capi.PHJ_ERR_INVALID


def test_python_names():
    assert "NO_ROW" in phj.__all__ and phj.NO_ROW == -1
    for name in ("join_indices", "joined_indices", "joined_indices_ptr", "joined_indices_to", "gather_column"):
        assert callable(getattr(phj.Context, name))


def test_cli_help_lists_rows():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    line = [ln for ln in r.stdout.splitlines() if "--rows" in ln]
    assert len(line) == 1 and "(=payloads)" in line[0] and "payloads | indices" in line[0]


def test_cli_rejects_unknown_rows_value(tmp_path):
    r = run(tmp_path, "--join-kind", "inner", "--rows", "xml")
    assert r.returncode == 1
    assert "the argument ('xml') for option '--rows' is invalid" in r.stdout


def test_cli_rows_indices_needs_rows_and_one_device(tmp_path):
    for extra in ([], ["--materialize", "on"], ["--aggregate", "totals"],
                  ["--join-kind", "full-outer", "--gpus", "2"], ["--materialize", "all", "--gpus", "2"],
                  ["--join-kind", "inner", "--exchange", "local"]):
        r = run(tmp_path, "--rows", "indices", *extra)
        assert r.returncode == 1, extra
        first = r.stdout.splitlines()[0]
        assert "--rows indices" in first or "--join-kind" in first or "--materialize" in first, (extra, first)
    # (`--rows payloads` is the default and goes with anything: refused for nothing)
    r = run(tmp_path, "--rows", "payloads", "--gpus", "99")
    assert r.returncode == 1 and "--gpus takes 1..16" in r.stdout.splitlines()[0]
