"""Relations bound as columns: what can be checked without a GPU. The new C
ABI symbols and their Python names exist, phj_relation_info has its documented
size, every new call refuses a null context before touching a device, and the
CLI knows --layout."""
import ctypes as C
import os
import subprocess

import partitionedhashjoin_amd as phj
from partitionedhashjoin_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "partitionedhashjoin_amd", "phjoin")
NEW = ["phj_relation_upload_columns", "phj_relation_bind_columns", "phj_relation_to_columns",
       "phj_relation_columns", "phj_relation_info_get"]


def test_symbols_exported_and_listed():
    L = _capi.load()
    for name in NEW:
        assert name in _capi.EXPORTED
        assert hasattr(L, name)
    header = open(os.path.join(ROOT, "include", "phj.h")).read()
    for name in NEW + ["PHJ_LAYOUT_TUPLES", "PHJ_LAYOUT_COLUMNS", "phj_relation_info"]:
        assert name in header
    assert "#define PHJ_ABI_VERSION 2" in header


def test_relation_info_layout():
    assert C.sizeof(_capi.RelationInfo) == 24
    assert [f[0] for f in _capi.RelationInfo._fields_] == ["n", "layout", "has_payloads", "packed", "owned"]
    assert (_capi.LAYOUT_TUPLES, _capi.LAYOUT_COLUMNS) == (0, 1)


def test_null_context_is_invalid():
    L = _capi.load()
    info = _capi.RelationInfo()
    k, p, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
    assert L.phj_relation_upload_columns(None, 0, None, None, 0) == _capi.PHJ_ERR_INVALID
    assert L.phj_relation_bind_columns(None, 0, None, None, 0) == _capi.PHJ_ERR_INVALID
    assert L.phj_relation_to_columns(None, 0, 1) == _capi.PHJ_ERR_INVALID
    assert L.phj_relation_columns(None, 0, C.byref(k), C.byref(p), C.byref(n)) == _capi.PHJ_ERR_INVALID
    assert L.phj_relation_info_get(None, 0, C.byref(info)) == _capi.PHJ_ERR_INVALID


def test_python_names():
    for name in ("RelationInfo", "LAYOUT_TUPLES", "LAYOUT_COLUMNS"):
        assert name in phj.__all__ and hasattr(phj, name)
    for name in ("upload_columns", "bind_columns", "to_columns", "columns_ptr", "relation_info"):
        assert callable(getattr(phj.Context, name))


def test_cli_rejects_unknown_layout():
    r = subprocess.run([CLI, "--join", "radix-partitioning", "--layout", "xml"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 1
    assert "the argument ('xml') for option '--layout' is invalid" in r.stdout


def test_cli_help_lists_layout():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    assert "--layout" in r.stdout and "tuples | columns" in r.stdout
